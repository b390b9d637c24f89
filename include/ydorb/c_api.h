/* ydorb C ABI — the drop-in boundary of the MI355X-native ORB / matcher / local-BA hot path.
 *
 * The reference (WeiZhang1988/YDORBSLAM) has no FFI layer: its hot path sits behind three C++
 * classes linked into libslam.so (src/CMakeLists.txt:14-31).  This header is the flat C ABI a
 * maintainer binds those classes to; the .hpp files next to this header are the adapter classes with the
 * reference's own signatures.  Every entry point cites the reference interface it replaces.
 *
 * Conventions: plain pointers + sizes, caller-owned buffers, opaque handles, int status return
 * (0 = YDORB_OK, <0 = error; ydorb_last_error() gives text).  No exceptions cross the ABI.
 * "d_" pointers are device (HBM) addresses, everything else is host memory.
 * A handle owns one HIP stream; distinct handles may be used concurrently from distinct threads
 * (the reference runs two extractors on two transient threads, src/frame.cpp:84-87).
 */
#ifndef YDORB_C_API_H
#define YDORB_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YDORB_OK 0
#define YDORB_ERR_INVALID_ARG -1
#define YDORB_ERR_NO_DEVICE -2     /* HIP runtime / gfx950 device not usable: there is NO CPU fallback */
#define YDORB_ERR_HIP -3           /* a HIP call failed */
#define YDORB_ERR_CAPACITY -4      /* caller buffer or internal scratch too small */
#define YDORB_ERR_UNSUPPORTED -5
#define YDORB_ERR_NUMERIC -6       /* BA: non-finite state */

const char* ydorb_last_error(void);
/* number of usable gfx950 devices (0 if none); never throws */
int ydorb_device_count(void);
const char* ydorb_version(void);

/* ------------------------------------------------------------------------------------------
 * cv::KeyPoint-compatible POD: 7 x 4 bytes, no padding (what extractAndCompute fills,
 * src/orbExtractor.cpp:355-399).
 * ---------------------------------------------------------------------------------------- */
typedef struct YdKeyPoint {
  float x, y;       /* pt, level-0 pixel units (level coords * scaleFactor[octave]) */
  float size;       /* (float)(int)(31 * scaleFactor[octave])   orbExtractor.cpp:595,600 */
  float angle;      /* degrees [0,360), cv::fastAtan2            orbExtractor.cpp:419 */
  float response;   /* FAST-9/16 corner score */
  int32_t octave;
  int32_t class_id; /* -1 */
} YdKeyPoint;

/* ------------------------------------------------------------------------------------------
 * ORB extractor.  Replaces YDORBSLAM::OrbExtractor (src/orbExtractor.hpp:31-74).
 * ---------------------------------------------------------------------------------------- */
typedef struct YdExtractorConfig {
  int32_t n_features;    /* OrbExtractor ctor args, src/orbExtractor.cpp:315-317 */
  float scale_factor;
  int32_t n_levels;      /* 1..8 */
  int32_t ini_fast_thr;
  int32_t min_fast_thr;  /* accepted and, like the reference (:318), replaced by ini_fast_thr */
  int32_t device;        /* HIP device ordinal */
  int32_t max_batch;     /* frames per launch the scratch is sized for (>=1) */
  int32_t flags;         /* YDORB_EXTRACTOR_* (0 = defaults) */
} YdExtractorConfig;
/* Every launch of a call goes on the one stream the call runs on (the quad-tree launches otherwise use two side streams of the handle
 * and overlap the blur: ~5 % faster alone).  For callers that pipeline several handles on several streams: the device has 4 hardware
 * queues, streams share them round-robin, and a side stream that lands behind another stream's long kernel stalls its handle. */
#define YDORB_EXTRACTOR_SINGLE_STREAM 1

typedef struct ydorb_extractor ydorb_extractor_t;

/* OrbExtractor::OrbExtractor, src/orbExtractor.cpp:315-354 */
int ydorb_extractor_create(const YdExtractorConfig* cfg, ydorb_extractor_t** out);
void ydorb_extractor_destroy(ydorb_extractor_t* h);

/* getScaleFactors / getInvScaleFactors / getScaleFactorSquares / getInvScaleFactorSquares and the
 * per-level keypoint quotas (src/orbExtractor.hpp:42-49, orbExtractor.cpp:325-339).  Each output may
 * be NULL; arrays hold n_levels entries. */
int ydorb_extractor_tables(const ydorb_extractor_t* h, float* scale, float* inv_scale, float* scale_sq,
                           float* inv_scale_sq, int32_t* per_level);
/* upper bound of keypoints one frame can return (sum of the per-level quotas) */
int ydorb_extractor_max_keypoints(const ydorb_extractor_t* h);

/* OrbExtractor::extractAndCompute(image, keypoints, descriptors), src/orbExtractor.cpp:355-399.
 * img: 8-bit gray, `stride` bytes per row (host).  kps/desc: caller buffers for `cap` keypoints
 * (desc is cap x 32 bytes, row-major like the CV_8U Mat at :373).  *n_out = keypoints written.
 * Empty image (w<=0||h<=0||!img) returns YDORB_OK with *n_out = 0, like :357-359. */
int ydorb_extract(ydorb_extractor_t* h, const uint8_t* img, int32_t w, int32_t hgt, int32_t stride,
                  YdKeyPoint* kps, uint8_t* desc, int32_t cap, int32_t* n_out);

/* Batched form of the same call: n_frames images of identical size, frame f at img + f*frame_stride.
 * Outputs: frame f's keypoints at kps + f*cap, descriptors at desc + f*cap*32, count at n_out[f]. */
int ydorb_extract_batch(ydorb_extractor_t* h, const uint8_t* img, int32_t w, int32_t hgt, int32_t stride,
                        size_t frame_stride, int32_t n_frames, YdKeyPoint* kps, uint8_t* desc, int32_t cap,
                        int32_t* n_out);

/* Device-resident batched form (inputs and outputs in HBM, asynchronous on the handle's stream or
 * on `stream` (a hipStream_t) when non-NULL; no host synchronisation).  cap must be >=
 * ydorb_extractor_max_keypoints().  d_n_out: int32[n_frames]. */
int ydorb_extract_batch_device(ydorb_extractor_t* h, const uint8_t* d_img, int32_t w, int32_t hgt, int32_t stride,
                               size_t frame_stride, int32_t n_frames, YdKeyPoint* d_kps, uint8_t* d_desc,
                               int32_t cap, int32_t* d_n_out, void* stream);
int ydorb_extractor_synchronize(ydorb_extractor_t* h);

/* m_v_imagePyramid[level] of the last call (public member read by src/frame.cpp:366,412-427):
 * device pointer to the level's ROI origin inside its 19-px reflect-101 padded buffer. */
int ydorb_extractor_pyramid(const ydorb_extractor_t* h, int32_t frame, int32_t level, const uint8_t** d_roi,
                            int32_t* w, int32_t* hgt, int32_t* stride);
/* Copy one padded level ((hgt+38) rows x (w+38) bytes, tightly packed) of the last call to host. */
int ydorb_extractor_read_level(ydorb_extractor_t* h, int32_t frame, int32_t level, uint8_t* dst, size_t dst_bytes);
/* All levels 0 .. n_levels-1 of one frame in ONE device-to-host transfer: dst_levels[l] receives (hgt_l+38) rows x (w_l+38) bytes,
 * tightly packed (the layout of ydorb_extractor_read_level).  This is what the adapter's m_v_imagePyramid refresh uses. */
int ydorb_extractor_read_pyramid(ydorb_extractor_t* h, int32_t frame, uint8_t* const* dst_levels, const size_t* dst_bytes, int32_t n_levels);

/* Test/diagnostic access to intermediate stages of the last call (parity tests compare each stage
 * with the oracle).  what: 0 = blurred level (hgt x w bytes), 1 = pre-quad-tree candidates
 * (YdKeyPoint[], border-relative coords as at orbExtractor.cpp:587-589), 2 = per-level keypoints after
 * orientation (YdKeyPoint[], level coords), 3 = one byte: which quad-tree kernel produced the (frame, level) unit
 * (0 = flat histogram/sort form, 1 = pass form; YDORB_QT_PASS=1 in the environment at create forces 1).
 * Returns bytes written in *written. */
int ydorb_extractor_debug_read(ydorb_extractor_t* h, int32_t what, int32_t frame, int32_t level, void* dst,
                               size_t dst_bytes, size_t* written);

/* Average device time (ms) of each pipeline stage over the calls since the last reset, measured with
 * HIP events on the handle's stream when profiling is enabled.  names: out array of static strings. */
int ydorb_extractor_set_profiling(ydorb_extractor_t* h, int32_t on);
int ydorb_extractor_stage_times(ydorb_extractor_t* h, int32_t max_stages, const char** names, float* ms,
                                int32_t* n_stages);

/* ------------------------------------------------------------------------------------------
 * Descriptor matcher.  Replaces YDORBSLAM::OrbMatcher (src/orbMatcher.hpp:24-66) for the
 * search-by-projection and search-by-BoW families.  Frame / KeyFrame / MapPoint objects do not cross the
 * ABI: a map point is a query row (descriptor + projected position + flags) and `assigned[idx]` stands
 * for frame.m_v_sptrMapPoints[idx] (a query index, or -1 for null).  The float geometry that projects map
 * points (cv::Mat products at orbMatcher.cpp:84-93,171-177) stays in the adapter class, which fills YdQuery
 * with the very floats the reference computes.  Frame::isInCameraFrustum (frame.cpp:295-326), the geometry of
 * Tracking::searchLocalPoints, is the exception: ydorb_frustum_cull and ydorb_search_local_points ("Local map
 * tracking" below) run it on the GPU.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdQuery {
  float u, v;          /* projected image position */
  float r;             /* radius given to Frame::getKeyPointsInArea (frame.cpp:337) */
  int32_t min_level, max_level; /* its _minScaleLevel/_maxScaleLevel arguments (-1 = open) */
  float ur;            /* projected right-image x; stereo test |ur - rightX[idx]| <= rs (orbMatcher.cpp:41,109) */
  float rs;
  float angle;         /* angle of the source keypoint (rotation histogram, orbMatcher.cpp:121) */
  int32_t level;       /* predicted / source scale level */
  int32_t flags;       /* bit0: query takes part; bit1: its map point has observations > 0 */
} YdQuery;

typedef struct YdFrameView {   /* the parts of YDORBSLAM::Frame the searches read (src/frame.hpp) */
  const YdKeyPoint* kps;       /* m_v_keyPoints (undistorted) */
  const uint8_t* desc;         /* m_cvMat_descriptors, n x 32 */
  const float* right_x;        /* m_v_rightXcords or NULL */
  int32_t n;
  float min_x, max_x, min_y, max_y; /* m_flt_minX.. (image bounds; the 64x48 grid spans them, frame.cpp:99-100) */
} YdFrameView;

typedef struct ydorb_matcher ydorb_matcher_t;
int ydorb_matcher_create(int32_t device, ydorb_matcher_t** out);
void ydorb_matcher_destroy(ydorb_matcher_t* h);

/* static int OrbMatcher::computeDescriptorsDistance(a, b), src/orbMatcher.cpp:11-23 (one pair, host). */
int ydorb_descriptor_distance(const uint8_t* a32, const uint8_t* b32);
/* The same distance for n row pairs on the GPU: out[i] = d(a[i], b[i]) (host pointers). */
int ydorb_descriptor_distance_rows(ydorb_matcher_t* h, const uint8_t* a, const uint8_t* b, int32_t n, int32_t* out);

/* Frame::getKeyPointsInArea, src/frame.cpp:337-361, on the GPU grid (ordered as the reference returns them). */
int ydorb_frame_keypoints_in_area(ydorb_matcher_t* h, const YdFrameView* frame, float x, float y, float r, int32_t min_level,
                                  int32_t max_level, int32_t* out_idx, int32_t cap, int32_t* n_out);

#define YDORB_SEARCH_FRAME_MAPPOINT 0   /* searchByProjectionInFrameAndMapPoint,       orbMatcher.cpp:24-64   */
#define YDORB_SEARCH_LAST_CURRENT 1     /* searchByProjectionInLastAndCurrentFrame,    orbMatcher.cpp:65-155  */
#define YDORB_SEARCH_KEYFRAME_CURRENT 2 /* searchByProjectionInKeyFrameAndCurrentFrame, orbMatcher.cpp:156-239 */
#define YDORB_SEARCH_SIM_PROJECTION 7   /* searchByProjectionInSim,                    orbMatcher.cpp:240-302 */
#define YDORB_SEARCH_BOW_KEYFRAME_FRAME 3 /* searchByBowInKeyFrameAndFrame,            orbMatcher.cpp:303-379 */
#define YDORB_SEARCH_BOW_TWO_KEYFRAMES 4  /* searchByBowInTwoKeyFrames,                orbMatcher.cpp:380-462 */

/* Projection family.  taken[idx] (in/out, n bytes): 1 where the frame keypoint already holds a map point that
 * blocks it (observations > 0 for modes 0/1, any map point for mode 2).  assigned[idx] (in/out, n ints): query
 * index written where the reference writes frame.m_v_sptrMapPoints[bestIdx]; untouched entries keep their value.
 * *n_matches = the int the reference returns (it counts overwrites and subtracts histogram culls exactly as
 * orbMatcher.cpp does).  * mode 7 = OrbMatcher::searchByProjectionInSim (orbMatcher.cpp:240-302, loop closing): the caller projects the map points with the
 * Sim3 it decomposed as the reference does; window without level check, explicit level window query.level-1 .. query.level, taken[idx] =
 * "_vSptrMatchedMapPoints[idx] is set" (a match takes its feature), best distance <= 50, no orientation check. */
int ydorb_search_by_projection(ydorb_matcher_t* h, int32_t mode, const YdFrameView* frame, const YdQuery* queries,
                               const uint8_t* qdesc, int32_t nq, float ratio, int32_t orb_dist, int32_t check_orientation,
                               uint8_t* taken, int32_t* assigned, int32_t* n_matches);

/* DBoW3::FeatureVector (std::map<node, vector<feature>>) as CSR: node_ids ascending, node_start[n_nodes+1], feat[]. */
typedef struct YdFeatureVector {
  const uint32_t* node_ids;
  const int32_t* node_start;
  const int32_t* feat;
  int32_t n_nodes;
} YdFeatureVector;
typedef struct YdBowSide {
  const YdKeyPoint* kps;
  const uint8_t* desc;
  const uint8_t* valid;   /* 1 where the feature has a good map point (may be NULL for the frame side of mode 3) */
  int32_t n;
  YdFeatureVector fv;
} YdBowSide;
/* BoW family.  mode 3: out[n_b] = keyframe-A feature whose map point goes to frame feature idx (or -1);
 * mode 4: out[n_a] = matched feature of keyframe B (or -1). */
int ydorb_search_by_bow(ydorb_matcher_t* h, int32_t mode, const YdBowSide* a, const YdBowSide* b, float ratio,
                        int32_t check_orientation, int32_t* out, int32_t* n_matches);


/* Search half of OrbMatcher::fuseByProjection (src/orbMatcher.cpp:682-745; fuseBySim3 :746-807 runs the same test on a
 * Sim3-projected point).  One query per map point that passed the reference's own predicates (not bad, not already in the keyframe,
 * in front of the camera, inside the image, inside the distance invariance, viewing angle — flags bit 0 set; other queries are
 * skipped): u, v = projection, r = th * scaleFactor[predicted level], ur = projected right x, level = predicted level.
 * best_idx[q] = the keyframe feature with the smallest descriptor distance (<= 50) among the window's features at level
 * predicted-1 .. predicted whose squared reprojection error passes the chi-square test (5.99 mono / 7.81 stereo), or -1.
 * The caller then walks the list in order and applies beReplacedBy / addObservation exactly as :726-737 (re-checking isBad /
 * isInKeyFrame at each step, because earlier replacements can change them; they cannot change a later point's search result). */
int ydorb_fuse_search(ydorb_matcher_t* h, const YdFrameView* keyframe, const YdQuery* queries, const uint8_t* qdesc, int32_t n_queries,
                      const float* inv_scale_factor_squares, int32_t n_levels, int32_t* best_idx, int32_t* n_found);
/* The same search with the acceptance distance as a parameter (ydorb_fuse_search = max_dist 50).  An all-zero inverse-sigma table
 * disables the chi-square test: that is fuseBySim3's search (orbMatcher.cpp:746-807) and, with max_dist = 100 (TH_HIGH), each of the two
 * directions of searchBySim3 (:594-667), whose agreement check (:668-679) the caller runs on the two result vectors. */
int ydorb_window_search(ydorb_matcher_t* h, const YdFrameView* keyframe, const YdQuery* queries, const uint8_t* qdesc, int32_t n_queries,
                        const float* inv_scale_factor_squares, int32_t n_levels, int32_t max_dist, int32_t* best_idx, int32_t* n_found);

/* OrbMatcher::searchForTriangulation (src/orbMatcher.cpp:463-565): BoW-guided search between the features of two
 * keyframes that have no MapPoint yet, kept when the second feature lies on the first one's epipolar line (:808-819).
 * has_map_point[i] != 0 <=> KeyFrame::getMapPoint(i) is set; right_x = m_v_rightXcords.  F = _fMatrix_first2second row-major
 * (F[r*3+c] = at<float>(r,c)); (epipole_x, epipole_y) = the first camera centre projected into the second image (:465-470, computed
 * by the caller exactly as the reference does); second_scale_factors / _squares = the second keyframe's m_v_scaleFactors /
 * m_v_scaleFactorSquares.  matched_second[first idx] = second idx or -1 (the reference's vector of pairs, in first-index order). */
typedef struct YdTriSide {
  const YdKeyPoint* kps;
  const uint8_t* desc;
  const float* right_x;
  const uint8_t* has_map_point;
  int32_t n;
  YdFeatureVector fv;
} YdTriSide;
int ydorb_search_for_triangulation(ydorb_matcher_t* h, const YdTriSide* first, const YdTriSide* second, const float* F, float epipole_x,
                                   float epipole_y, const float* second_scale_factors, const float* second_scale_factor_squares,
                                   int32_t n_levels, int32_t stereo_only, int32_t check_orientation, int32_t* matched_second,
                                   int32_t* n_matches);

/* MapPoint::computeDistinctiveDescriptors(), src/mapPoint.cpp:169-218, for a batch of map points.  Point p's descriptors (the
 * rows the member function collects at :183-187, in that order) are desc[offsets[p] .. offsets[p+1]); offsets[0] = 0.
 * best[p] = bestMedianIdx (:203-213): the first descriptor whose sorted distance row has the least entry at (int)(0.5 m);
 * -1 for a point without descriptors (the reference returns early, :188).  One map point per call is far below launch
 * latency - hand over all points of a LocalMapping / LoopClosing pass at once. */
int ydorb_distinctive_descriptors(ydorb_matcher_t* h, const uint8_t* desc, const int32_t* offsets, int32_t n_points, int32_t* best);

/* Frame::computeStereoMatches(), src/frame.cpp:362-477: for every left keypoint the best right descriptor among the right
 * keypoints whose row band covers its row, an 11x11 block match over 11 column shifts at the keypoint's pyramid level,
 * parabola refinement, disparity -> depth, and the final outlier rule.  One call handles n_pairs rectified pairs.
 * The image pyramids are those the two extractors built in their last call (m_v_imagePyramid, read at :366,412-427):
 * pair p reads frame first_frame + p*frame_step of that call on each side (so one batched extractor call over interleaved
 * left/right images, or two extractors, both work).  Keypoints are the undistorted ones (frame.cpp:91-93).
 * right_x / depth: float [n_pairs][left->cap] = m_v_rightXcords / m_v_depth (-1 = none, -2 = removed by the outlier rule).
 * n_kept[p] = entries of vDistIndices; status[p]: bit0 = a left keypoint's (int)pt.y was outside [0, rows) (undefined vector
 * index in the reference; counted as a row without right keypoints), bit1 = a block-match window started left of the image
 * (cv::Exception in the reference; treated like the other window `continue`s).  Either may be NULL.
 * flags: default 0 replays the reference as written, including its left index that only advances when a keypoint reaches
 * the end of the loop body (:462) - a serial chain over the keypoints of a pair; YDORB_STEREO_INDEX_BY_KEYPOINT uses the
 * keypoint's own index for the descriptor row and the output slot (one wave per keypoint).  With
 * YDORB_STEREO_DEVICE_POINTERS every array argument is a device pointer and the call is asynchronous on `stream`
 * (a hipStream_t) or the matcher's own, ordered by the caller after the extractor calls. */
#define YDORB_STEREO_INDEX_BY_KEYPOINT 1
#define YDORB_STEREO_DEVICE_POINTERS 2
typedef struct YdStereoSide {
  const ydorb_extractor_t* extractor;
  int32_t first_frame, frame_step;
  const YdKeyPoint* kps;  /* [n_pairs][cap] */
  const uint8_t* desc;    /* [n_pairs][cap][32] */
  const int32_t* n;       /* [n_pairs] */
  int32_t cap;            /* right side: <= 8192 */
  int32_t reserved;
} YdStereoSide;
int ydorb_stereo_matches(ydorb_matcher_t* h, const YdStereoSide* left, const YdStereoSide* right, int32_t n_pairs, float bf, float b,
                         int32_t flags, float* right_x, float* depth, int32_t* n_kept, int32_t* status, void* stream);

/* Device-resident streaming form used after ydorb_extract_batch_device: for f = 0..n_frames-2, the keypoints of
 * frame f are searched in frame f+1 with the searchByProjectionInLastAndCurrentFrame rules (mode 1; position
 * prediction = d_affine[f] (2x3, row-major) applied to the keypoint, NULL = identity; window th*scaleFactor[octave];
 * levels octave-1..octave+1).  d_assigned: int32 [n_frames-1][cap] (query index per frame-f+1 keypoint or -1),
 * d_counts: int32 [n_frames-1].  Asynchronous on `stream` (or the matcher's own). */
int ydorb_match_consecutive_device(ydorb_matcher_t* h, const YdKeyPoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                   int32_t cap, int32_t n_frames, int32_t width, int32_t height, float th,
                                   const float* scale_factors, int32_t n_levels, const float* d_affine, int32_t check_orientation,
                                   int32_t* d_assigned, int32_t* d_counts, void* stream);
/* The same search for an explicit list of (query frame, target frame) pairs over two device-resident frame sets (which may be the
 * same set): pair p searches the keypoints of queries[pairs[2p]] in targets[pairs[2p+1]].  This is the form the multi-GPU path
 * uses after the all-gather of every rank's [keypoints | descriptors | count] records: targets = the gathered set of all ranks,
 * queries = the frames whose successor this rank owns; greedy acceptance stays with the owner of the target frame.
 * `pairs` is a host array; both sets must use the same cap.  d_assigned: int32 [n_pairs][cap] indexed by target keypoint,
 * d_counts: int32 [n_pairs], d_affine: [n_pairs][6] or NULL.  Asynchronous on `stream` (or the matcher's own). */
typedef struct YdFrameSetDev {
  const YdKeyPoint* d_kps;  /* [n_frames][cap] */
  const uint8_t* d_desc;    /* [n_frames][cap][32] */
  const int32_t* d_n;       /* [n_frames] */
  int32_t n_frames, cap;
} YdFrameSetDev;
int ydorb_match_pairs_device(ydorb_matcher_t* h, const YdFrameSetDev* queries, const YdFrameSetDev* targets, const int32_t* pairs,
                             int32_t n_pairs, int32_t width, int32_t height, float th, const float* scale_factors, int32_t n_levels,
                             const float* d_affine, int32_t check_orientation, int32_t* d_assigned, int32_t* d_counts, void* stream);
/* Brute-force 256-bit Hamming top-2 (BASELINE north_star).  For every query descriptor the result of the reference's
 * best / second-best chain (orbMatcher.cpp:39-52 and the same chain at :327-334, :404-417, :518-528) over its candidates in list
 * order: best = the FIRST candidate with the least distance, second = the first one with the least distance among the others;
 * both start at 256 and only a strictly smaller distance replaces them (dist 256 / index -1 = none).  *_rank = position in the
 * query's candidate list (what breaks ties), *_idx = the target row.
 * Host form: q [nq][32], t [nt][32]; candidates of query i = cand_idx[cand_offsets[i] .. cand_offsets[i+1]) (CSR), or - with
 * cand_offsets == cand_idx == NULL - all nt targets in index order.  nt <= 65535 per list. */
typedef struct YdMatch2 {
  int32_t best_dist, best_idx, second_dist, second_idx, best_rank, second_rank;
} YdMatch2;
int ydorb_hamming_topk(ydorb_matcher_t* h, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, const int32_t* cand_offsets,
                       const int32_t* cand_idx, YdMatch2* out);
/* Device-resident all-pairs form for n_pairs (query frame, target frame) pairs laid out [n_pairs][cap][32] with per-pair counts:
 * d_out [n_pairs][cap] YdMatch2.  Asynchronous on `stream` (or the matcher's own). */
int ydorb_hamming_topk_device(ydorb_matcher_t* h, const uint8_t* d_qdesc, const int32_t* d_nq, const uint8_t* d_tdesc, const int32_t* d_nt,
                              int32_t cap, int32_t n_pairs, YdMatch2* d_out, void* stream);
int ydorb_matcher_synchronize(ydorb_matcher_t* h);
/* average device ms of grid build / gather / resolve over calls since enabling (HIP events on the launch stream) */
int ydorb_matcher_set_profiling(ydorb_matcher_t* h, int32_t on);
int ydorb_matcher_stage_times(ydorb_matcher_t* h, int32_t max_stages, const char** names, float* ms, int32_t* n_stages);
/* ydorb_mapdb_create_new_points with profiling on: ms [3] = average device ms per call of the join and gather, of the resolve
 * launches of the chain and of its geometry launches (an event after every launch); n_calls = the calls averaged. */
int ydorb_matcher_create_points_times(ydorb_matcher_t* h, float* ms, int32_t* n_calls);

/* ------------------------------------------------------------------------------------------
 * Vocabulary.  Replaces DBoW3::Vocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
 * (thirdParty/DBow3/src/Vocabulary.cpp:752-824; descent :836-874) as called by Frame::computeBoW / KeyFrame::computeBoW
 * (src/frame.cpp:265-272, levelsup = 4).  The tree crosses the boundary once, as flat arrays (the adapter flattens
 * Vocabulary::m_nodes): node 0 is the root, node i's children are child_ids[child_begin[i] .. child_begin[i+1]) in the order of
 * Node::children (that order breaks distance ties: first minimum, :858-865); a node without children is a word.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdVocabularyTree {
  int32_t n_nodes;
  int32_t levels;              /* m_L */
  const int32_t* child_begin;  /* [n_nodes + 1] */
  const int32_t* child_ids;    /* [child_begin[n_nodes]] */
  const uint8_t* node_desc;    /* [n_nodes][32]  Node::descriptor (the root's row is not read) */
  const double* node_weight;   /* [n_nodes]      Node::weight (read for words) */
  const int32_t* node_word;    /* [n_nodes]      Node::word_id (read for words) */
  int32_t weighting;           /* WeightingType: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY */
  int32_t norm;                /* what the scoring object's mustNormalize() asks for: 0 none, 1 L1, 2 L2 */
} YdVocabularyTree;
typedef struct ydorb_vocabulary ydorb_vocabulary_t;
int ydorb_vocabulary_create(const YdVocabularyTree* tree, int32_t device, ydorb_vocabulary_t** out);
void ydorb_vocabulary_destroy(ydorb_vocabulary_t* h);
/* One call transforms n_frames descriptor sets (frame f: n[f] <= cap rows at desc + f*cap*32; cap <= 8192).
 * BowVector of frame f: bow_word / bow_value [f*cap .. + n_words[f]) in ascending word id (std::map order), values exactly as the
 * reference's sequence of additions and its normalisation produce them (doubles).  FeatureVector of frame f as the CSR that
 * YdFeatureVector takes: fv_node [f*cap .. + n_fv_nodes[f]) ascending, fv_start [f*(cap+1) ..] offsets into fv_feat [f*cap ..].
 * status[f] (may be NULL) bit0: a descent ended above level L - levelsup, where the reference reads its `nid` uninitialised
 * (Vocabulary.cpp:777,868); such a feature is filed under the leaf's own node id.  Calls on one handle from several threads are
 * serialised inside (the reference shares one vocabulary between its tracking, local-mapping and loop-closing threads). */
int ydorb_vocabulary_transform(ydorb_vocabulary_t* h, const uint8_t* desc, const int32_t* n, int32_t n_frames, int32_t cap, int32_t levelsup,
                               int32_t* bow_word, double* bow_value, int32_t* n_words, int32_t* fv_node, int32_t* fv_start, int32_t* fv_feat,
                               int32_t* n_fv_nodes, int32_t* status);

/* ------------------------------------------------------------------------------------------
 * Local bundle adjustment.  Replaces the g2o work inside
 *   static void Optimizer::localBundleAdjust(shared_ptr<KeyFrame>, shared_ptr<Map>, bool& stop)   src/optimizer.cpp:138-352
 * (and the shared BA kernel of Optimizer::bundleAdjust, :7-137).  The covisibility walk that collects local /
 * fixed keyframes and map points (:140-173) and the write-back under Map::m_mutex_updateMap (:336-351) stay in the
 * adapter; this call receives the flat graph that :175-283 would hand to g2o and runs :284-334 on the GPU:
 * optimize(5) with Huber kernels -> mark edges with chi2 > 5.991 (mono) / 7.815 (stereo) or non-positive depth and drop
 * the kernels -> optimize(10) on the inliers -> final outlier list.
 * Precondition: at most ONE edge per (pose, point) pair, fixed poses included.  The reference cannot produce two: a map point's
 * observations are a std::map<shared_ptr<KeyFrame>, size_t> (MapPoint::getObservations(), walked at optimizer.cpp:232-282), one
 * entry per keyframe.  A problem that repeats a pair is refused with YDORB_ERR_INVALID_ARG on the host, before any kernel runs
 * and with poses / points untouched (ydorb_ba_solve, every member of ydorb_ba_solve_batch on its own, every rank of a sharded solve).
 * ---------------------------------------------------------------------------------------- */
typedef struct YdBaProblem {
  int32_t n_poses, n_points, n_edges;
  double* poses;                 /* [n_poses][7] tx,ty,tz,qx,qy,qz,qw = g2o::SE3Quat of T_c2w (Converter, converter.cpp:12-19); in/out */
  const uint8_t* pose_fixed;     /* [n_poses] setFixed(): keyframe id 0 and the "fixed keyframes" (optimizer.cpp:191,204) */
  double* points;                /* [n_points][3] world position; in/out */
  const int32_t* edge_pose;      /* [n_edges] index into poses */
  const int32_t* edge_point;     /* [n_edges] index into points */
  const double* edge_meas;       /* [n_edges][3] u, v, u_right; u_right < 0 selects the monocular 2-D edge (optimizer.cpp:239) */
  const double* edge_inv_sigma2; /* [n_edges] m_v_invScaleFactorSquares[octave] (information = I * this, :248,268) */
  double fx, fy, cx, cy, bf;     /* Frame::m_flt_* statics (:254-257, :275-279) */
  const volatile uint8_t* stop;  /* the reference's `bool& _bIsStopping`; NULL = the null-reference default (optimizer.hpp:34) */
} YdBaProblem;

typedef struct YdBaOptions {
  int32_t iters1, iters2;        /* 5 and 10 (optimizer.cpp:288,314) */
  double chi2_mono, chi2_stereo; /* 5.991, 7.815 (:296,306) */
  double delta_mono, delta_stereo; /* Huber delta: (double)(float)sqrt(5.991|7.815) (:223-224) */
  int32_t max_trials;            /* maxTrialsAfterFailure = 10 (optimization_algorithm_levenberg.cpp:50) */
  int32_t device;
  /* multi-GPU (landmarks sharded over ranks, every rank holds all poses): called on device buffer d_buf holding
   * `count` doubles; op 0 = sum, 1 = max over ranks.  NULL = single GPU. */
  int32_t (*allreduce)(void* user, void* d_buf, int64_t count, int32_t op);
  void* allreduce_user;
  void* d_comm_buf;              /* device workspace the callback can address (e.g. a torch tensor), >= comm_doubles doubles */
  int64_t comm_doubles;
  int32_t rank, world;
  int32_t flags;                 /* YDORB_BA_* bits below; 0 = localBundleAdjust's two-stage schedule */
  int32_t reserved;
} YdBaOptions;
/* Optimizer::bundleAdjust / globalBundleAdjust (optimizer.cpp:7-137, :353-357) use the same graph and solver with ONE
 * optimize(iters1) call: no chi2 cull, no second stage (edge_outlier is still filled with the chi2/depth test for the caller's
 * information), Huber kernels optional (_bIsRobust) and delta_mono = (double)(float)sqrt(5.99) — note 5.99, :37. */
#define YDORB_BA_SINGLE_STAGE 1
#define YDORB_BA_NO_ROBUST 2
/* fill YdBaResult.ms_errors .. ms_update: a pair of stream events round every phase of every LM trial, ~10 us of stream time each
 * (8 % of a 100-keyframe solve), so the breakdown is opt-in; ms_total is always measured */
#define YDORB_BA_PHASE_TIMES 4
/* TEST ONLY, honoured by ydorb_ba_solve_batch alone: every upload of the per-problem round record is preceded on the batch's stream
 * by a host function that sleeps 200 us, so that the copy reads its pinned source long after the host has gone on.  A host write
 * into an area whose upload is still in flight then shows as a wrong result instead of once in a long while.  At most two uploads
 * per round, a few dozen rounds per group. */
#define YDORB_BA_TEST_LATE_UPLOADS 8

typedef struct YdBaResult {
  int32_t n_trials;              /* LM trials executed (each = linearise/Schur/solve/update/chi2) */
  int32_t n_iterations;          /* outer LM iterations over both stages */
  int32_t n_log;
  int32_t stopped;               /* 1 if the stop flag ended the run early */
  double log_chi2[32];           /* robust chi2 after each outer iteration */
  double log_lambda[32];
  int32_t log_trials[32];
  int32_t log_stage[32];
  uint8_t* edge_outlier;         /* [n_edges] caller buffer: 1 = erase the observation (optimizer.cpp:316-334); may be NULL */
  float ms_total, ms_errors, ms_build, ms_schur, ms_solve, ms_update; /* device time per phase, summed over trials (HIP events) */
} YdBaResult;

/* default options as the reference uses them */
void ydorb_ba_default_options(YdBaOptions* opt);
/* Re-entrant: every call takes one of 8 per-device contexts (own stream and scratch), so several host threads — several maps or
 * sessions — may solve at once; a ninth concurrent caller waits.  Results do not depend on what else runs (fixed summation
 * orders).  The reference itself calls localBundleAdjust from one thread (localMapping.cpp:29). */
int ydorb_ba_solve(const YdBaProblem* prob, const YdBaOptions* opt, YdBaResult* res);
/* n independent problems (several maps / sessions / replayed windows) solved in LOCK STEP: one set of kernel launches per phase for
 * all problems (blockIdx.z = problem), the LM state of every problem kept on the host exactly as in ydorb_ba_solve and decided once per
 * round from ONE read-back.  One solve is a latency chain of ~35 small launches per LM trial that leaves most of the GPU idle; a
 * batch costs about the time of its slowest member plus the throughput-bound kernels.  `threads` = problems advanced together
 * (0 = up to 64 per group; larger batches run group after group).  The problems may differ in every size.  res[i] / rc_each[i]
 * (may be NULL) per problem; returns the first non-zero status.  Every result is bit-identical to its own ydorb_ba_solve call. */
int ydorb_ba_solve_batch(const YdBaProblem* probs, int32_t n, const YdBaOptions* opt, YdBaResult* res, int32_t threads, int32_t* rc_each);

/* The solver keeps its device scratch between calls: 8 contexts per device for ydorb_ba_solve / ydorb_pose_optimize and up to 64
 * problem contexts (~40 MB each at 100 keyframes x 10 000 points) for ydorb_ba_solve_batch.  ydorb_ba_release frees all of it on `device`
 * (waiting for solves in flight); the next call allocates again.  The reference has no counterpart: g2o's optimizer dies with
 * localBundleAdjust's stack frame (optimizer.cpp:175-181). */
int ydorb_ba_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * Pose-only optimisation.  Replaces YDORBSLAM::Optimizer::optimizePose (src/optimizer.cpp:358-501) — the
 * Tracking thread calls it 1-3x per frame right after a match (tracking.cpp:386,466,611).  A batch of frames is solved in one
 * launch, one workgroup per frame running all four episodes.  Frame f owns edges [edge_start[f], edge_start[f+1]): one per
 * keypoint that has a map point; points = MapPoint::getPosInWorld() (world), meas = (kp.x, kp.y, rightX or < 0 for monocular),
 * inv_sigma2 = m_v_invScaleFactorSquares[kp.octave].  poses [n][7] = (t, unit q) of T_c2w, in/out.
 * Outputs: outlier[e] = Frame::m_v_isOutliers of the edge's keypoint, n_inliers[f] = the function's return value
 * (initialCorrespondenceNum - badNum; 0 and an untouched pose when a frame has < 3 edges), optional chi2_log [n][4] (robust chi2
 * after each episode, NaN where an episode did not run) and trials [n] (LM trials executed). */
typedef struct YdPoseBatch {
  int32_t n_frames;
  int32_t device;
  const int32_t* edge_start;     /* [n_frames + 1] */
  double* poses;                 /* [n_frames][7] in/out */
  const double* points;          /* [n_edges][3] */
  const double* meas;            /* [n_edges][3] */
  const double* inv_sigma2;      /* [n_edges] */
  double fx, fy, cx, cy, bf;
} YdPoseBatch;
int ydorb_pose_optimize(const YdPoseBatch* batch, uint8_t* outlier, int32_t* n_inliers, double* chi2_log, int32_t* trials);

/* dense SPD solve with the BA's blocked Cholesky (known-answer tests; A is n x n row-major, host pointers) */
int ydorb_ba_dense_solve(int32_t device, const double* A, int32_t n, const double* b, double* x, int32_t* ok);

/* The reduced camera system's second solver.  DENSE holds S as (6 nPf)^2 doubles, nPf the free poses, and stops
 * at dense_max_rows = 19 200 rows, 3 200 free keyframes.  SKYLINE holds the envelope of S's 6x6 blocks under an order of the free
 * poses: memory and work follow the covisibility band, the pose-pair buckets are the covisible pairs + nPf instead of
 * nPf (nPf + 1) / 2, and nothing is sized by nPf^2.  AUTO is DENSE whenever 6 nPf <= dense_max_rows and SKYLINE above: a call that
 * succeeded before returns the same bytes, a call that was refused now succeeds.  `ordering` is YDORB_ESS_ORDER_SMALLER / NATURAL /
 * RCM (below, "Essential graph").  SKYLINE is refused with YDORB_ERR_UNSUPPORTED on the host, before any kernel runs and before the
 * stage's device memory is sized (ydorb_ba_plan gives the same answer without touching a device),
 *   - when world > 1 (the all-reduce of S stays dense only);
 *   - when the envelope takes more than max_factor_bytes (0 = 19 200^2 * 8 B, the largest dense S);
 *   - when the factorisation takes more than 2^24 block updates per trial (sum over the block columns of m (m + 1) / 2, m = the rows
 *     below the diagonal that reach the column; 432 flop each, 7.2e9 flop): one workgroup walks the columns in one launch that
 *     nothing can interrupt, and section 6j allows such a launch 1.2e10 flop.
 * The error text names the size and the limit.  ydorb_ba_solve is ydorb_ba_solve_with(DENSE); ydorb_ba_solve_batch stays dense only. */
enum { YDORB_BA_SOLVER_AUTO = 0, YDORB_BA_SOLVER_DENSE = 1, YDORB_BA_SOLVER_SKYLINE = 2 };
typedef struct YdBaSolverOptions {
  int32_t solver, ordering;
  int64_t max_factor_bytes;      /* 0 = default */
} YdBaSolverOptions;
typedef struct YdBaSolverInfo {
  int32_t solver_used, ordering_used, n_free, max_row_blocks, dense_max_rows, reserved;
  int64_t covisible_pairs;       /* pairs of free poses that share a landmark; the skyline path has covisible_pairs + n_free buckets */
  int64_t envelope_blocks, envelope_blocks_natural, envelope_blocks_rcm;
  int64_t pair_updates;          /* block updates of one factorisation */
  int64_t factor_bytes;          /* of S as the solver used holds it */
} YdBaSolverInfo;
/* Host only, touches no device: the solver a solve of `prob` would use and its plan.  perm [n_free] (free pose at each position of
 * the order) and first [n_free] (first block column of each row) may be NULL.  NULL sopt = AUTO. */
int ydorb_ba_plan(const YdBaProblem* prob, const YdBaOptions* opt, const YdBaSolverOptions* sopt, YdBaSolverInfo* info, int32_t* perm,
                  int32_t* first);
/* ydorb_ba_solve with the solver chosen; info may be NULL.  NULL sopt = AUTO. */
int ydorb_ba_solve_with(const YdBaProblem* prob, const YdBaOptions* opt, const YdBaSolverOptions* sopt, YdBaResult* res, YdBaSolverInfo* info);
/* TEST / DEBUG: one linearisation at the given estimate and one Schur complement with `lambda` (not range-checked: a negative one
 * must give *solved = 0), S expanded on the host to [6F][6F] full symmetric in the caller's free-pose order, bs [6F] and the solve
 * x [6F].  Refused when 6F > 4096.  prob is not written. */
int ydorb_ba_reduced_system_with(const YdBaProblem* prob, const YdBaOptions* opt, const YdBaSolverOptions* sopt, double lambda,
                                 double* S_out, double* bs_out, double* x_out, int32_t* solved);
/* TEST / DEBUG: the counterpart of ydorb_ba_dense_solve.  A is n x n row-major, n a multiple of 6 and <= 4096; the block pattern is
 * the set of non-zero 6x6 blocks of A. */
int ydorb_ba_skyline_solve(int32_t device, const double* A, int32_t n, const double* b, int32_t ordering, double* x, int32_t* ok);

/* ------------------------------------------------------------------------------------------
 * Sim3 RANSAC of the loop-closure check.  Replaces Sim3Solver::iterate (ORB-SLAM2 src/Sim3Solver.cc: iterate, ComputeSim3,
 * CheckInliers, Project) for a batch of candidate keyframes; LoopClosing::computeSim3 calls it with chunk 5 per candidate.
 * The constructor's work (camera-frame points, their images, maxError = 9.210 * sigma^2) and setRansacParameters stay with the
 * caller (include/ydorb/sim3Solver.hpp), which hands over the N kept pairs.  The RANSAC's index triples are inputs, drawn by the
 * caller in the reference's order (RandomInt over the available-index copy, then swap-remove): the reference draws them from the
 * process-global rand(), so the result is a pure function of the arguments.  One call runs what repeated iterate(chunk) calls do
 * from next_hyp on: it stops at the first hypothesis with inliers >= the running best AND > min_inliers (the reference's return),
 * at max_its, or when the triples run out.  fp32 arithmetic in the written order of DESIGN.md section 2 ("Sim3 RANSAC"): the
 * result is bit-identical to a CPU restatement compiled with -ffp-contract=off.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdSim3Problem {
  int32_t n;                     /* kept pairs N (mvX3Dc1.size()) */
  int32_t fix_scale;             /* mbFixScale */
  int32_t min_inliers, max_its;  /* mRansacMinInliers, mRansacMaxIts as setRansacParameters left them */
  const float* X1;               /* [n][3] mvX3Dc1: KF1's points in KF1's camera frame */
  const float* X2;               /* [n][3] mvX3Dc2 */
  const float* P1;               /* [n][2] mvP1im1: X1 through K1 */
  const float* P2;               /* [n][2] mvP2im2 */
  const float* max_err1;         /* [n] mvnMaxError1 */
  const float* max_err2;         /* [n] mvnMaxError2 */
  float K1[4], K2[4];            /* fx, fy, cx, cy */
  int32_t n_hyp;                 /* triples supplied: hypotheses next_hyp .. next_hyp + n_hyp - 1 */
  const int32_t* triples;        /* [n_hyp][3] indices into the n pairs, in draw order */
  int32_t next_hyp;              /* in/out: mnIterations */
  int32_t best_inliers;          /* in/out: mnBestInliers */
  float best_T12[13];            /* in/out: mBestT12 as R (row-major 3x3), t, s; on a return = the returned T12 */
  int32_t ret_hyp;               /* out: global index of the hypothesis at which iterate returns, -1 if none */
  int32_t no_more;               /* out: bNoMore of the last iterate(chunk) call the sequence ran */
  int32_t n_calls;               /* out: iterate(chunk) calls the sequence ran */
  int32_t reserved;
  uint8_t* inliers;              /* out [n]: the returned inlier set over the pairs (all 0 without a return) */
  int32_t* hyp_inliers;          /* out [n_hyp], may be NULL: inlier count of every evaluated hypothesis (-1 where none ran) */
} YdSim3Problem;
int ydorb_sim3_ransac(YdSim3Problem* probs, int32_t n_probs, int32_t chunk, int32_t device);

/* Optimizer::optimizeSim3 (ORB-SLAM2 Optimizer::OptimizeSim3, src/Optimizer.cc) for a batch of problems, one workgroup per problem:
 * one VertexSim3Expmap (g2o sim3.h exp map, _fix_scale), two projection edges per pair (EdgeSim3ProjectXYZ against obs1,
 * EdgeInverseSim3ProjectXYZ against obs2, information I * inv_sigma2, Huber delta sqrtf(th2), central-difference Jacobians with
 * delta 1e-9) -> optimize(5) -> drop pairs with chi2 > th2 on either edge -> return 0 if fewer than 10 pairs remain -> optimize(nBad ?
 * 10 : 5) -> count.  Problem p owns pairs [corr_start[p], corr_start[p+1]).  Outputs: outlier[pair] (the pairs the reference sets to
 * NULL), n_in[p] (the return value; S12 untouched when it is 0 by the early return), optional chi2_log [n][2] (robust chi2 after each
 * optimize, NaN where it did not run) and trials [n] (LM trials over both stages). */
typedef struct YdSim3Batch {
  int32_t n_problems;
  int32_t device;
  const int32_t* corr_start;     /* [n_problems + 1] */
  double* S12;                   /* [n_problems][8] qx, qy, qz, qw, tx, ty, tz, s; in/out */
  const double* K1;              /* [n_problems][4] fx, fy, cx, cy of KF1 */
  const double* K2;              /* [n_problems][4] of KF2 */
  const uint8_t* fix_scale;      /* [n_problems] */
  const double* X1c;             /* [pairs][3] KF1's point in KF1's camera frame */
  const double* X2c;             /* [pairs][3] KF2's point in KF2's camera frame */
  const double* obs1;            /* [pairs][2] kpUn1 */
  const double* obs2;            /* [pairs][2] kpUn2 */
  const double* inv_sigma2_1;    /* [pairs] KF1->mvInvLevelSigma2[kpUn1.octave] */
  const double* inv_sigma2_2;    /* [pairs] */
  double th2;                    /* the reference's float th2 (10 in loop closing) */
} YdSim3Batch;
int ydorb_sim3_optimize(const YdSim3Batch* batch, uint8_t* outlier, int32_t* n_in, double* chi2_log, int32_t* trials);

/* Both Sim3 entries keep device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_sim3_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * EPnP RANSAC of relocalisation.  Replaces PnPsolver::iterate (ORB-SLAM2 src/PnPsolver.cc: iterate, Refine, CheckInliers and
 * Lepetit's EPnP compute_pose) for a batch of candidate keyframes; Tracking::relocalize calls it with chunk 5 per candidate.
 * The constructor's work (the N kept matches: world points, undistorted keypoints, maxError = sigma^2 * th2) and
 * setRansacParameters stay with the caller (include/ydorb/pnpSolver.hpp).  The 4-point sets are inputs, drawn by the caller in the
 * reference's order (RandomInt over the available-index copy, then swap-remove).  One call runs what repeated iterate(chunk) calls do
 * from next_hyp on: it stops at the first hypothesis whose Refine succeeds, at the end of the call that sets bNoMore, or when the
 * quads run out.  fp64 EPnP in the written order of DESIGN.md section 2 ("EPnP RANSAC"): the result is bit-identical to a CPU
 * restatement compiled with -ffp-contract=off.
 * ---------------------------------------------------------------------------------------- */
#define YDORB_PNP_NONE 0      /* iterate returned an empty Mat */
#define YDORB_PNP_REFINED 1   /* returned Refine's pose at hypothesis ret_hyp */
#define YDORB_PNP_BEST 2      /* returned the unrefined best pose when the iterations ran out */
typedef struct YdPnpProblem {
  int32_t n;                     /* kept matches N (mvP2D.size()) */
  int32_t min_inliers, max_its;  /* mRansacMinInliers, mRansacMaxIts as setRansacParameters left them */
  int32_t loop_or;               /* 1: while (mnIterations < maxIts || nCurrent < nIterations) (ORB-SLAM2); 0: the && variant */
  const float* Xw;               /* [n][3] mvP3Dw */
  const float* P2D;              /* [n][2] mvP2D */
  const float* max_err;          /* [n] mvMaxError */
  float K[4];                    /* fu, fv, uc, vc */
  int32_t n_hyp;                 /* quads supplied: hypotheses next_hyp .. next_hyp + n_hyp - 1 */
  const int32_t* quads;          /* [n_hyp][4] indices into the n matches, in draw order */
  int32_t next_hyp;              /* in/out: mnIterations */
  int32_t best_inliers;          /* in/out: mnBestInliers */
  uint8_t* best_mask;            /* in/out [n]: mvbBestInliers (the next Refine reads it) */
  float best_Tcw[12];            /* in/out: mBestTcw, rows 0..2 of the 4x4 (row-major 3x4) */
  int32_t ret_hyp;               /* out: global index of the hypothesis whose Refine returned, -1 otherwise */
  int32_t ret_how;               /* out: YDORB_PNP_NONE / _REFINED / _BEST */
  int32_t no_more;               /* out: bNoMore of the last iterate(chunk) call the sequence ran */
  int32_t n_calls;               /* out: iterate(chunk) calls the sequence ran */
  float Tcw[12];                 /* out: the returned pose (3x4 row-major), zeros with YDORB_PNP_NONE */
  int32_t n_inliers;             /* out: nInliers */
  int32_t reserved;
  uint8_t* inliers;              /* out [n]: the returned inlier set over the matches (all 0 without a return) */
  int32_t* hyp_inliers;          /* out [n_hyp], may be NULL: inlier count of every evaluated hypothesis (-1 where none ran) */
} YdPnpProblem;
int ydorb_pnp_ransac(YdPnpProblem* probs, int32_t n_probs, int32_t chunk, int32_t device);

/* ydorb_pnp_ransac keeps device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_pnp_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * KeyFrameDatabase: place-recognition queries.  Replaces KeyFrameDatabase (ORB-SLAM2 src/KeyFrameDatabase.cc; YDORBSLAM
 * keyFrameDatabase.*) and the DBoW3::Vocabulary::score calls (ScoringObject.cpp) in it and in LoopClosing::detectLoop.  The database
 * keeps the BowVector of every key frame in HBM; a key frame is known by the slot ydorb_kfdb_add returned.  BowVectors travel in CSR
 * form: start [n + 1] (start[0] = 0), word ids ascending and unique within a vector (std::map order), double values: the layout
 * ydorb_vocabulary_transform emits.  A query of more than 8192 words is YDORB_ERR_UNSUPPORTED.  Results are bit-identical to a CPU
 * restatement compiled with -ffp-contract=off.  Calls on one handle are serialised inside.
 * ---------------------------------------------------------------------------------------- */
typedef struct ydorb_kfdb ydorb_kfdb_t;
/* DBoW3::ScoringType.  KL and BHATTACHARYYA are refused with YDORB_ERR_UNSUPPORTED ("unsupported scoring"): they need log(), which
 * is not bit-reproducible between host libm and the device. */
#define YDORB_KFDB_L1_NORM 0
#define YDORB_KFDB_L2_NORM 1
#define YDORB_KFDB_CHI_SQUARE 2
#define YDORB_KFDB_KL 3
#define YDORB_KFDB_BHATTACHARYYA 4
#define YDORB_KFDB_DOT_PRODUCT 5
/* status word of a relocalisation query */
#define YDORB_KFDB_STALE_SCORE 1       /* a neighbour's mRelocScore came from an earlier query (it shares a word but was not scored now) */
#define YDORB_KFDB_UNWRITTEN_SCORE 2   /* a neighbour's mRelocScore was never written; the reference reads an uninitialised float, here 0.0f */

/* KeyFrameDatabase(voc): scoring = the vocabulary's ScoringType; the capacities are initial sizes, storage grows. */
int ydorb_kfdb_create(int32_t device, int32_t scoring, int32_t slot_capacity, int64_t word_capacity, ydorb_kfdb_t** out);
void ydorb_kfdb_destroy(ydorb_kfdb_t* db);
/* KeyFrameDatabase::add for n key frames: appends each to the database in the given order (the order of the inverted file's lists).
 * slots [n] out.  A slot freed by erase may be handed out again; the new key frame is a new one in every respect. */
int ydorb_kfdb_add(ydorb_kfdb_t* db, const int32_t* start, const int32_t* word, const double* value, int32_t n, int32_t* slots);
/* KeyFrameDatabase::erase */
int ydorb_kfdb_erase(ydorb_kfdb_t* db, const int32_t* slots, int32_t n);
/* KeyFrameDatabase::clear */
int ydorb_kfdb_clear(ydorb_kfdb_t* db);
/* key frames in the database and slots in use (the length of the diagnostic arrays); either may be NULL */
int ydorb_kfdb_size(ydorb_kfdb_t* db, int32_t* n_live, int32_t* n_slots);
/* KeyFrame::getBestCovisibilityKeyFrames(10) of n key frames, as the queries read it: neigh [n][10] slots in the reference's order,
 * -1 padded.  A neighbour that is not in the database is dropped; one erased later is skipped from then on. */
int ydorb_kfdb_set_covisibility(ydorb_kfdb_t* db, const int32_t* slots, const int32_t* neigh, int32_t n);
/* DBoW3::Vocabulary::score(query, key frame) for n slots: LoopClosing::detectLoop's minimum-score loop over the connected key frames. */
int ydorb_kfdb_score(ydorb_kfdb_t* db, const int32_t* q_word, const double* q_value, int32_t n_words, const int32_t* slots, int32_t n,
                     double* scores);
/* KeyFrameDatabase::detectRelocalizationCandidates for n_queries frames, equal to that many single calls in order (mRelocScore of a
 * key frame carries over from query to query and from call to call).  cand [n_queries][cand_cap]: the returned key frames' slots in
 * the reference's order; counts [n_queries]: their number (when it exceeds cand_cap only the first cand_cap are written); status
 * [n_queries], may be NULL: YDORB_KFDB_* bits.  diag_words / diag_score [slots in use], both NULL or both set: common words and
 * (float)score of the LAST query against every key frame that shares a word with it, 0 elsewhere. */
int ydorb_kfdb_detect_reloc(ydorb_kfdb_t* db, const int32_t* q_start, const int32_t* q_word, const double* q_value, int32_t n_queries,
                            int32_t* cand, int32_t cand_cap, int32_t* counts, int32_t* status, int32_t* diag_words, float* diag_score);
/* KeyFrameDatabase::detectLoopCandidates(pKF, minScore) for n_queries key frames: conn_start [n_queries + 1] / conn_slots = each
 * query's pKF->getConnectedKeyFrames() (slots; key frames outside the database are left out), min_score [n_queries]. */
int ydorb_kfdb_detect_loop(ydorb_kfdb_t* db, const int32_t* q_start, const int32_t* q_word, const double* q_value, int32_t n_queries,
                           const int32_t* conn_start, const int32_t* conn_slots, const float* min_score, int32_t* cand, int32_t cand_cap,
                           int32_t* counts, int32_t* status, int32_t* diag_words, float* diag_score);

/* ------------------------------------------------------------------------------------------
 * LocalMapping::createNewMapPoints: the geometry between searchForTriangulation's match list and the new MapPoints (ORB-SLAM2
 * LocalMapping::CreateNewMapPoints' inner loop, which YDORBSLAM renames): ray and stereo parallax, the 4x4 linear
 * triangulation or the stereo unprojection, both depth tests, both reprojection chi-square tests and the scale-consistency test, one
 * GPU lane per match.  A batch holds n_problems keyframe pairs over n_views shared views (one current keyframe meets 10-20
 * neighbours); problem p pairs views first_view[p] / second_view[p] and owns the matches match_start[p] .. match_start[p+1] of idx1
 * (keypoint of the first view) / idx2 (of the second).  Results are bit-identical to a CPU restatement compiled with
 * -ffp-contract=off ("createNewMapPoints").
 * ---------------------------------------------------------------------------------------- */
typedef struct YdTriView {      /* one keyframe */
  const YdKeyPoint* kps;        /* [n] m_v_keyPoints (x, y and octave are read) */
  const float* right_x;         /* [n] m_v_rightXcords: >= 0 marks a stereo feature */
  const float* depth;           /* [n] m_v_depth */
  int32_t n;
  float Tcw[12];                /* 3x4 row-major; Rwc = Rcw^T and Ow as the reference's getters return them: */
  float Rwc[9], Ow[3];
  float fx, fy, cx, cy, invfx, invfy, b, bf;
  const float* level_sigma2;    /* [n_levels] m_v_scaleFactorSquares */
  const float* scale_factors;   /* [n_levels] m_v_scaleFactors */
  int32_t n_levels;
} YdTriView;
typedef struct YdTriBatch {
  int32_t device, n_views, n_problems;
  const YdTriView* views;
  const int32_t* first_view; const int32_t* second_view;   /* [n_problems] */
  const int32_t* match_start;                              /* [n_problems+1], match_start[0] = 0, non-decreasing */
  const int32_t* idx1; const int32_t* idx2;                /* [match_start[n_problems]] */
  const float* ratio_factor;                               /* [n_problems] = 1.5f * first view's scale factor */
} YdTriBatch;
/* status byte of a match.  Low nibble = where the reference's loop body left (0 = it reached the new MapPoint): */
#define YDORB_TRI_ACCEPTED 0
#define YDORB_TRI_NO_METHOD 1        /* neither the linear nor a stereo branch applies */
#define YDORB_TRI_W_ZERO 2           /* homogeneous w == 0 */
#define YDORB_TRI_DEPTH_FIRST 3      /* z1 <= 0 */
#define YDORB_TRI_DEPTH_SECOND 4     /* z2 <= 0 */
#define YDORB_TRI_REPROJ_FIRST 5
#define YDORB_TRI_REPROJ_SECOND 6
#define YDORB_TRI_ZERO_DISTANCE 7
#define YDORB_TRI_SCALE_RATIO 8
#define YDORB_TRI_BAD_STEREO_DEPTH 9 /* the stereo unprojection was chosen for a feature whose depth is not > 0 (undefined in the reference) */
/* bits 4-5 = the source of x3d: */
#define YDORB_TRI_SRC_LINEAR 1
#define YDORB_TRI_SRC_UNPROJECT_FIRST 2
#define YDORB_TRI_SRC_UNPROJECT_SECOND 3
#define YDORB_TRI_NOT_FINITE 0x80    /* bit 7: a component of x3d is NaN or infinite (the reference's tests are all false on NaN: such a point is accepted) */
/* x3d [M][3], status [M] with M = match_start[n_problems]; n_accepted [n_problems] or NULL.  x3d[m] is the triangulated / unprojected
 * point whenever a source produced one, for rejected matches too, and 0 0 0 otherwise (exits 1, 2 and 9).  Null arrays, a view or a
 * keypoint index out of range, an octave outside [0, n_levels) of a referenced keypoint and a malformed match_start return
 * YDORB_ERR_INVALID_ARG before any device work. */
int ydorb_triangulate_matches(const YdTriBatch* batch, float* x3d, uint8_t* status, int32_t* n_accepted);
/* ydorb_triangulate_matches keeps device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_triangulate_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * Local map tracking: Tracking::searchLocalPoints (tracking.cpp:570-604), i.e. Frame::isInCameraFrustum (frame.cpp:295-326) per
 * local map point with MapPoint::predictScaleLevel, then searchByProjectionInFrameAndMapPoint (orbMatcher.cpp:24-64).  The
 * semantics restate ORB-SLAM2's Frame::isInFrustum and MapPoint::PredictScale, which YDORBSLAM renames; DESIGN.md section 2
 * ("isInCameraFrustum") fixes the fp32 operation order and lists the assumptions.  One GPU lane per (view, map point); results are
 * bit-identical to a CPU restatement compiled with -ffp-contract=off.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdFrustumView {  /* one frame: pose, intrinsics, image bounds and the scale pyramid */
  float Rcw[9], tcw[3], Ow[3];  /* m_cvMat_R_c2w row-major, m_cvMat_t_c2w, m_cvMat_origin: as the frame holds them */
  float fx, fy, cx, cy, bf;
  float min_x, max_x, min_y, max_y;
  float viewing_cos_limit;      /* 0.5 in searchLocalPoints */
  int32_t n_levels;             /* 1..8 */
  float level_ratio[7];         /* [n_levels-1] used: level_ratio[k] = the largest float ratio for which
                                   ceil(log(ratio) / logScaleFactor) <= k; the predicted level is the number of entries strictly below
                                   maxDistance / dist.  Built on the host with the reference's own log (tracking.hpp levelRatioTable) */
  float scale_factors[8];       /* m_v_scaleFactors; read by ydorb_search_local_points only */
} YdFrustumView;
typedef struct YdMapPointTable { /* the map points shared by all views of a call */
  const float* pos_min;         /* [n][4]: getPosInWorld() x y z, getMinDistanceInvariance() */
  const float* normal_max;      /* [n][4]: getNormal() x y z, getMaxDistanceInvariance() */
  const float* max_distance;    /* [n]: the raw m_flt_maxDistance (predictScaleLevel divides it by the distance) */
  const uint8_t* desc;          /* [n][32] getDescriptor(); read by ydorb_search_local_points only, may be NULL otherwise */
  int32_t n;
} YdMapPointTable;
typedef struct YdFrustumBatch {
  int32_t device, n_views;
  const YdFrustumView* views;   /* [n_views] */
  YdMapPointTable table;
  const int32_t* list_start;    /* [n_views+1], list_start[0] = 0, non-decreasing: view f tests entries list_start[f] .. list_start[f+1] */
  const int32_t* point_idx;     /* [list_start[n_views]] index into the table */
  const uint8_t* skip;          /* [list_start[n_views]] 1 = the caller skips this point (isBad(), or last seen in this frame) */
} YdFrustumBatch;
typedef struct YdTrackView {    /* what isInCameraFrustum leaves on a map point in view; all zero otherwise */
  float u, v, ur, view_cos;     /* m_flt_trackProjX, m_flt_trackProjY, m_flt_trackProjRightX, m_flt_trackViewCos */
  int32_t level;                /* m_int_trackScaleLevel */
} YdTrackView;
/* status byte of a list entry: the first exit that fires, in the reference's order */
#define YDORB_FRUSTUM_IN_VIEW 0
#define YDORB_FRUSTUM_SKIPPED 1     /* the caller's skip flag */
#define YDORB_FRUSTUM_BEHIND 2      /* PcZ < 0.0f */
#define YDORB_FRUSTUM_OUT_U 3       /* u < minX || u > maxX */
#define YDORB_FRUSTUM_OUT_V 4       /* v < minY || v > maxY */
#define YDORB_FRUSTUM_DISTANCE 5    /* dist < minDistInv || dist > maxDistInv */
#define YDORB_FRUSTUM_VIEW_ANGLE 6  /* viewCos < viewingCosLimit */
/* rows [L], status [L] with L = list_start[n_views]; n_in_view [n_views] or NULL.  A NaN passes every exit and PcZ == 0 gives inf / NaN
 * projections that fail no bounds test, as in the reference.  Null arrays, a malformed list_start, a point index outside the table
 * and n_levels outside 1..8 return YDORB_ERR_INVALID_ARG before any device work. */
int ydorb_frustum_cull(const YdFrustumBatch* batch, YdTrackView* rows, uint8_t* status, int32_t* n_in_view);
/* ydorb_frustum_cull keeps device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_frustum_release(int32_t device);
/* Tracking::searchLocalPoints' numeric part in one call.  The result is defined as the composition of (1) ydorb_frustum_cull with one
 * view over the points 0 .. table->n-1 (skip [n]), (2) the query build of searchByProjectionInFrameAndMapPoint (orbMatcher.cpp:28-38):
 * radius = th * (view_cos > 0.998 ? 2.5f : 4.0f), r = rs = radius * scale_factors[level], level window level-1 .. level, flags =
 * 1 | (has_observations[i] ? 2 : 0), flags = 0 for points not in view, and (3) ydorb_search_by_projection(mode 0, ratio) with
 * table->desc as the queries' descriptors; the queries are built on the device and never visit the host.  taken / assigned as in
 * ydorb_search_by_projection (assigned[idx] = point index); rows [n], status [n] as in ydorb_frustum_cull; *n_to_match = the number
 * of points in view (the reference searches only when it is > 0: with 0, *n_matches = 0 and assigned is untouched). */
int ydorb_search_local_points(ydorb_matcher_t* h, const YdFrameView* frame, const YdFrustumView* view, const YdMapPointTable* table,
                              const uint8_t* skip, const uint8_t* has_observations, float th, float ratio, uint8_t* taken,
                              int32_t* assigned, YdTrackView* rows, uint8_t* status, int32_t* n_to_match, int32_t* n_matches);

/* ------------------------------------------------------------------------------------------
 * Frame construction.  The tail of the RGB-D Frame constructor after extractAndCompute (src/frame.cpp:99-100,134-145):
 * undistortKeyPoints, computeStereoFromRGBD, computeImageBounds and assignKeyPointsToGrid.  The reference source is restated from
 * ORB-SLAM2's Frame::UndistortKeyPoints / ComputeStereoFromRGBD / ComputeImageBounds / AssignFeaturesToGrid, which YDORBSLAM renames;
 * DESIGN.md section 2 ("Frame tail: the arithmetic contract") states the arithmetic and lists what a maintainer with the reference
 * must check.  Its undistorted keypoints are what every matcher entry above takes as "the undistorted ones".
 * ---------------------------------------------------------------------------------------- */
typedef struct YdCamera {       /* m_cvMat_intParMat and m_cvMat_distCoef as floats (frame.cpp:134-145) */
  float fx, fy, cx, cy;
  float dist[5];                /* k1 k2 p1 p2 k3 */
  int32_t n_iter;               /* iterations of cv::undistortPoints: 5 = its public overload's criterion; >= 1 */
} YdCamera;
/* Undistortion, in fp64 on floats widened to double: x0 = x = (u - cx) * (1.0 / fx), y0 = y = (v - cy) * (1.0 / fy); n_iter times
 * r2 = x x + y y, icdist = 1.0 / (1.0 + ((k3 r2 + k2) r2 + k1) r2), [icdist < 0: x = x0, y = y0, stop, status bit 2],
 * dX = 2.0 p1 x y + p2 (r2 + 2.0 x x), dY = p1 (r2 + 2.0 y y) + 2.0 p2 x y, x = (x0 - dX) icdist, y = (y0 - dY) icdist; the result is
 * (float)(fx x + cx), (float)(fy y + cy).  k1 == 0.0f copies the points, whatever the other coefficients are (frame.cpp:134-145). */
/* xy, xy_out: float [n][2] (host).  frame.cpp:134-145 */
int ydorb_undistort_points(const YdCamera* cam, const float* xy, int32_t n, float* xy_out, int32_t device);
/* Frame::computeImageBounds, frame.cpp:99-100: the corners (0,0) (w,0) (0,h) (w,h) through the undistortion above, on the device;
 * bounds = min_x, max_x, min_y, max_y = min(c0.x, c2.x), max(c1.x, c3.x), min(c0.y, c1.y), max(c2.y, c3.y); k1 == 0: 0, w, 0, h. */
int ydorb_image_bounds(const YdCamera* cam, int32_t w, int32_t hgt, float* bounds, int32_t device);

#define YDORB_DEPTH_NONE 0      /* monocular tail: right_x = depth = -1 */
#define YDORB_DEPTH_U16 1       /* uint16 image, d = (float)raw * depth_factor (imDepth.convertTo(CV_32F, factor)) */
#define YDORB_DEPTH_F32 2       /* float image, as it is */
#define YDORB_DEPTH_SAMPLES 3   /* float [n_frames][cap]: one scaled sample per keypoint, gathered by the caller */
#define YDORB_FRAME_DEPTH_AT_UNDISTORTED 1 /* index the depth image with the undistorted keypoint (default: the raw one) */
#define YDORB_FRAME_DEVICE_POINTERS 2      /* every array is a device pointer; asynchronous on `stream` */
#define YDORB_FRAME_STATUS_DEPTH_INDEX 1   /* status bit 0: a keypoint's depth pixel lay outside the image (no depth) */
#define YDORB_FRAME_STATUS_ICDIST 4        /* status bit 2: icdist < 0 ended a keypoint's undistortion */
typedef struct YdFrameTail {
  const YdKeyPoint* kps;        /* [n_frames][cap] as extracted */
  const int32_t* n;             /* [n_frames], each <= cap */
  int32_t n_frames, cap;
  const void* depth;            /* image of frame f at depth + f * depth_frame_stride bytes; samples: float [n_frames][cap]; NULL with NONE */
  int32_t depth_type;           /* YDORB_DEPTH_* */
  int32_t depth_w, depth_h;     /* image forms */
  int64_t depth_row_stride;     /* bytes per image row, >= depth_w elements */
  int64_t depth_frame_stride;   /* bytes between the images of consecutive frames */
  float depth_factor;           /* U16 only (m_flt_depthMapFactor) */
  float bf;                     /* m_flt_baseLineTimesFx */
  YdCamera cam;
  float bounds[4];              /* min_x, max_x, min_y, max_y of ydorb_image_bounds; read for the grid only */
  int32_t flags;                /* YDORB_FRAME_* */
  int32_t device;
} YdFrameTail;
/* frame.cpp:134-145 for a batch of frames.  Outputs, each may be NULL and is then skipped: kps_un [n_frames][cap] (the other keypoint
 * fields are copied); right_x, depth [n_frames][cap] = m_v_rightXcords / m_v_depth: the depth pixel is ((int)kp.y, (int)kp.x) of the
 * raw keypoint, truncating (a coordinate in (-1, size) is inside; anything else, NaN included, is an unchecked Mat::at in the
 * reference and gives no depth and status bit 0 here); d > 0 gives depth = d, right_x = un.x - bf / d (float), anything else -1 / -1;
 * cell_start [n_frames][3073], cell_idx [n_frames][cap]: the 64x48 grid of kps_un as a CSR, cell ix * 48 + iy, indices ascending in
 * a cell, keypoints outside the grid left out, with the matcher's cell rule (it rounds and offsets y by min_x); status [n_frames].
 * Slots n .. cap of an output are unspecified.  Host form: one upload, the kernels, one read-back, one synchronise.  With
 * YDORB_FRAME_DEVICE_POINTERS the call is asynchronous on `stream` (a hipStream_t, or the tail's own when NULL), ordered by the caller
 * behind ydorb_extract_batch_device; it does not synchronise and allocates nothing after the first call of a size; kps_un is then what
 * ydorb_match_consecutive_device / YdFrameSetDev take.  cap <= 65535 when the grid is asked for. */
int ydorb_frame_tail(const YdFrameTail* tail, YdKeyPoint* kps_un, float* right_x, float* depth, int32_t* cell_start, int32_t* cell_idx,
                     int32_t* status, void* stream);
/* The RGB-D constructor's device work in one call, on one stream with one synchronise (frame.cpp:99-100,134-145 behind
 * extractAndCompute): upload of gray and depth, ydorb_extract_batch_device, the tail kernels, one read-back; the extractor's capacity
 * status (ydorb_extractor_synchronize on its then idle streams) is checked behind it.  depth: image of the
 * gray image's size with depth_stride bytes per row, depth_type NONE (or depth NULL: the monocular tail), U16 or F32.  kps_raw, desc,
 * n_out as ydorb_extract fills them; the remaining outputs as ydorb_frame_tail's for one frame, each may be NULL (bounds may be NULL
 * when no grid is asked for).  An empty image returns YDORB_OK with *n_out = 0. */
int ydorb_extract_rgbd(ydorb_extractor_t* h, const uint8_t* gray, int32_t w, int32_t hgt, int32_t stride, const void* depth,
                       int32_t depth_type, int32_t depth_stride, float depth_factor, const YdCamera* cam, float bf, const float* bounds,
                       int32_t flags, YdKeyPoint* kps_raw, YdKeyPoint* kps_un, uint8_t* desc, float* right_x, float* depth_out,
                       int32_t* cell_start, int32_t* cell_idx, int32_t cap, int32_t* n_out, int32_t* status);
/* The frame-construction entries keep device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_frame_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * Essential-graph optimisation of loop closing.  Replaces Optimizer::optimizeEssentialGraph (ORB-SLAM2
 * Optimizer::OptimizeEssentialGraph, src/Optimizer.cc): one VertexSim3Expmap per keyframe, EdgeSim3 edges with identity information
 * and no robust kernel (error = log(Sji * Siw * Sjw^-1)), BaseBinaryEdge's numeric Jacobians (delta 1e-9), Levenberg-Marquardt with
 * setUserLambdaInit(lambda_init), optimize(iterations), then the map-point correction.  The graph (which keyframes, which edges) is
 * built by the caller (include/ydorb/optimizer.hpp).  Two solvers factorise the normal equations (7 rows per free vertex):
 *   DENSE    assembled dense and factorised by the BA's blocked Cholesky.  Its limit: more than 19 200 / 7 = 2 742 free vertices return
 *            YDORB_ERR_UNSUPPORTED.  ydorb_essential_graph_optimize / _trial_step always take it.
 *   SKYLINE  a block-skyline Cholesky over the envelope of the 7x7 blocks: no limit on the vertex count; its
 *            limit is the envelope's size in bytes, YdEssentialSolverOptions::max_factor_bytes (default: the largest dense matrix,
 *            19 200^2 * 8).  The bytes bound the memory only; one workgroup walks the factor, so a second, fixed limit bounds the work:
 *            more than 2^24 block updates per trial (the sum over the block columns of m (m + 1) / 2, m = the rows that reach the
 *            column: a dense envelope of 465 keyframes, or a band of 6 over a million) return YDORB_ERR_UNSUPPORTED as well.
 *            Chosen through the _with entries below.
 * fp64 under the contract of DESIGN.md section 2 ("Essential graph: the arithmetic contract"); two calls on the same graph with the
 * same solver and ordering give the same bits.
 * Checked before any device work (YDORB_ERR_INVALID_ARG): null arrays, a vertex index outside 0..n_vertices-1, edge_v0 == edge_v1,
 * no fixed vertex, every vertex fixed, non-positive iterations / max_trials / lambda_init / scale (vertex or measurement).
 * An edge between two fixed vertices counts in chi2 only; a repeated pair is legal and summed in edge order.
 * res: the iteration log as the single-stage BA writes it (log_stage = 1; edge_outlier is not used); ms_build / ms_schur / ms_solve /
 * ms_update / ms_errors = device time of linearize / assemble / factorise + solve / update / trial chi2 when
 * ydorb_essential_graph_set_profiling switched the event pairs on (they cost a few microseconds per launch), 0 otherwise.
 * points_out [n_points][3] = float(correctedSwr.map(Srw.map(double(points[p])))) with Srw the reference vertex's estimate as it came
 * in and correctedSwr the inverse of its estimate as it goes out; may be NULL when n_points == 0.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdEssentialGraph {
  int32_t device, n_vertices, n_edges, n_points;
  double* sim3;             /* [n_vertices][8] qx qy qz qw tx ty tz s: initial estimate in (vScw), optimised estimate out */
  const uint8_t* fixed;     /* [n_vertices] 1 = the loop keyframe's vertex */
  const int32_t* edge_v0;   /* [n_edges] vertex(0) = i */
  const int32_t* edge_v1;   /* [n_edges] vertex(1) = j */
  const double* edge_meas;  /* [n_edges][8] Sji */
  const float* points;      /* [n_points][3] world positions, may be NULL when n_points == 0 */
  const int32_t* point_ref; /* [n_points] vertex of the reference (or correcting) keyframe */
  int32_t fix_scale, iterations /* 20 */, max_trials /* 10 */;
  double lambda_init;       /* 1e-16: setUserLambdaInit */
} YdEssentialGraph;
int ydorb_essential_graph_optimize(const YdEssentialGraph* g, float* points_out, YdBaResult* res);
/* TEST / DEBUG: linearises the graph once at the estimate handed in (same argument checks, nothing is optimised or written back) and
 * returns what k_ess_linearize stored: err [n_edges][7], J0 and J1 [n_edges][7][7] (row = error component, column = update dimension;
 * zero for a fixed vertex) and chi2 [n_edges].  Each output may be NULL. */
int ydorb_essential_graph_linearize(const YdEssentialGraph* g, double* err, double* J0, double* J1, double* chi2);
/* TEST / DEBUG: the solve of one LM trial at the estimate handed in (same argument checks, nothing is written back): linearise,
 * assemble H + lambda I, factorise, solve.  x [7 * free vertices] = the update the trial would apply, free vertices in vertex order;
 * *solved = 0 when a pivot was not positive (x is then not a solution). */
int ydorb_essential_graph_trial_step(const YdEssentialGraph* g, double lambda, double* x, int32_t* solved);
/* 1: ydorb_essential_graph_optimize on `device` fills the ms_* fields of its result from HIP event pairs; 0 (default): no events. */
int ydorb_essential_graph_set_profiling(int32_t device, int32_t on);
/* The entries keep device scratch and, once profiling was on, ten HIP events per device between calls; this frees them (waiting for a
 * call in flight). */
int ydorb_essential_graph_release(int32_t device);

/* The choice of solver.  AUTO: DENSE whenever the graph fits the dense limit (every call that succeeds through the entries above then
 * returns the same bytes), SKYLINE above it.  DENSE above its limit fails as above.  ordering (SKYLINE): the order of the free vertices
 * in the factor, NATURAL = the caller's, RCM = reverse Cuthill-McKee (pseudo-peripheral start, ties by vertex index, components by their
 * lowest vertex), SMALLER = the one with the smaller envelope, NATURAL on a tie.  A NULL options pointer means all zeros. */
enum { YDORB_ESS_SOLVER_AUTO = 0, YDORB_ESS_SOLVER_DENSE = 1, YDORB_ESS_SOLVER_SKYLINE = 2 };
enum { YDORB_ESS_ORDER_SMALLER = 0, YDORB_ESS_ORDER_NATURAL = 1, YDORB_ESS_ORDER_RCM = 2 };
typedef struct YdEssentialSolverOptions {
  int32_t solver, ordering;
  int64_t max_factor_bytes; /* 0 = default */
} YdEssentialSolverOptions;
/* What was planned: the envelope counts 7x7 blocks (392 bytes each), a row from its first connected column to the diagonal.
 * ordering_used is NATURAL or RCM; envelope_blocks / max_row_blocks (the longest row) belong to it.  factor_bytes: the matrix the
 * solver used holds (DENSE: the padded square). */
typedef struct YdEssentialSolverInfo {
  int32_t solver_used, ordering_used, n_free, max_row_blocks;
  int64_t envelope_blocks, envelope_blocks_natural, envelope_blocks_rcm, factor_bytes;
} YdEssentialSolverInfo;
/* Host only, no device is touched: the argument checks of ydorb_essential_graph_optimize, then the order and the envelope.
 * perm [free vertices]: perm[k] = the free vertex (counted in vertex order) at position k of the factor; first [free vertices]:
 * first[k] = the first column of row k's envelope, by position.  Either may be NULL.  YDORB_ERR_UNSUPPORTED (the text names both
 * sizes) when SKYLINE is asked for and the envelope exceeds max_factor_bytes or the work limit, or DENSE above its limit. */
int ydorb_essential_graph_plan(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, YdEssentialSolverInfo* info, int32_t* perm,
                               int32_t* first);
/* ydorb_essential_graph_optimize with the solver chosen; info may be NULL.  With DENSE it is that entry. */
int ydorb_essential_graph_optimize_with(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, float* points_out, YdBaResult* res,
                                        YdEssentialSolverInfo* info);
/* TEST / DEBUG: ydorb_essential_graph_trial_step with the solver chosen and any lambda (it is not range-checked here: a negative one
 * makes a pivot non-positive, *solved = 0).  H_out [7F][7F] (F free vertices, caller's vertex order, full symmetric) and b_out [7F]:
 * copies of the assembled H, without lambda, and of b, whichever solver stored them; either may be NULL; 7F > 4096 is refused. */
int ydorb_essential_graph_trial_step_with(const YdEssentialGraph* g, const YdEssentialSolverOptions* opt, double lambda, double* x,
                                          int32_t* solved, double* H_out, double* b_out);

/* ------------------------------------------------------------------------------------------
 * Map maintenance: the three passes over the observation table (map point -> the keyframes that observe it) that run between
 * processNewKeyFrame and the next keyframe.  They restate ORB-SLAM2's MapPoint::UpdateNormalAndDepth, the counting loop of
 * KeyFrame::UpdateConnections and the counting of LocalMapping::KeyFrameCulling (YDORBSLAM: updateNormalAndDepth, updateConnections,
 * keyFrameCulling).  The reference source is absent from this repository: the semantics are restated from ORB-SLAM2, and DESIGN.md
 * section 2 ("Map maintenance") fixes the fp32 operation order.  Assumptions for a maintainer who holds the reference to check:
 *   - normal / double is OpenCV's scale by 1./s, applied to CV_32F data with a float factor;
 *   - the observation container iterates in an address-dependent order, so this ABI takes the order and the adapter passes the
 *     container's own;
 *   - the scale factors are one pyramid for all keyframes;
 *   - thObs = 3, a stereo observation weighs 2 in observations(), the covisibility threshold is 15, the culling verdict is the
 *     double compare nRedundant > 0.9 * nMPs, and culling skips the first keyframe of the map (the caller omits it).
 * All three read one flattened table, local to the call; keyframe slots 0 .. n_keyframes-1 are chosen by the caller.  Integer
 * results are exact and the fp32 results are bit-identical to a CPU restatement compiled with -ffp-contract=off.
 * Every malformed input returns YDORB_ERR_INVALID_ARG before any device work, the message naming the first offender: null arrays, a
 * *_start that does not begin at 0 or decreases, a slot or point index out of range, a level >= n_levels where scale_factors is
 * read, device outside 0..15.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdObservationTable {
  int32_t n_points, n_keyframes;
  const int32_t* obs_start;   /* [n_points+1], obs_start[0] = 0, non-decreasing */
  const int32_t* obs_kf;      /* [N] observing keyframe slot, in the iteration order of the reference's observation map */
  const uint8_t* obs_level;   /* [N] bits 0-6: octave of the observing keypoint; bit 7: stereo observation (right x >= 0) */
  const uint8_t* bad;         /* [n_points] isBad() */
} YdObservationTable;
/* status byte of a map point */
#define YDORB_MAP_UPDATED 0
#define YDORB_MAP_BAD 1              /* isBad(): the reference returns before it reads anything */
#define YDORB_MAP_NO_OBSERVATIONS 2  /* the observation map is empty: the reference returns */
/* MapPoint::updateNormalAndDepth for every point of the table.  pos [n_points][3]; centre [n_keyframes][3] = the camera origins;
 * ref_kf / ref_level [n_points] = the reference keyframe's slot and the octave of its observing keypoint (read for updated points
 * only); scale_factors [n_levels], n_levels in 1..8.  normal [n_points][3], min_distance / max_distance [n_points] are the raw
 * members (not the 0.8x / 1.2x getters), all zero for a point that is not updated.  A point at an observer's centre gives NaN
 * components, as in the reference. */
int ydorb_map_update_normal_depth(const YdObservationTable* table, const float* pos, const float* centre, const int32_t* ref_kf,
                                  const uint8_t* ref_level, const float* scale_factors, int32_t n_levels, int32_t device, float* normal,
                                  float* min_distance, float* max_distance, uint8_t* status);
/* The counter map of KeyFrame::updateConnections for n_queries keyframes.  query_kf [n_queries] slots; list_start [n_queries+1] /
 * point_idx = each keyframe's non-null map-point entries (a point listed twice counts twice); out_start [n_queries+1] = where each
 * query's results go and how many fit (min(n_keyframes - 1, sum of the listed points' spans) always fits).  Bad points and the
 * query's own slot are skipped.  Per query: conn_kf / conn_weight [out_start[q] .. + counts[q]) = the keyframes with a non-zero
 * count, ascending by slot; counts [n_queries]; status [n_queries]: 0 = ok, 1 = capacity too small (nothing is written for that
 * query, counts holds the needed size).  The threshold of 15, the keep-the-best rule and the sort stay with the caller. */
int ydorb_map_covisibility(const YdObservationTable* table, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                           const int32_t* point_idx, const int32_t* out_start, int32_t device, int32_t* conn_kf, int32_t* conn_weight,
                           int32_t* counts, uint8_t* status);
/* The counting of LocalMapping::keyFrameCulling for n_candidates keyframes.  cand_kf [n_candidates] slots; list_start
 * [n_candidates+1] / point_idx / own_level = each candidate's entries whose map point is non-null and whose depth passes
 * !(depth > thDepth || depth < 0) (the caller's float test), with the octave of the candidate's own keypoint; removed
 * [n_keyframes] or NULL = keyframes culled since the table was flattened; th_obs = 3.  With w(p) = the sum over p's observers not
 * in `removed` of (stereo ? 2 : 1), an entry is skipped when bad[p], or when p has an observer in `removed` and w(p) <= 2 (what
 * eraseObservation does to such a point); otherwise it counts into n_counted, and into n_redundant when w(p) > th_obs and at least
 * th_obs observers other than the candidate, not removed, have level <= own_level + 1.
 * cull[k] = (double)n_redundant[k] > 0.9 * (double)n_counted[k]. */
int ydorb_map_keyframe_redundancy(const YdObservationTable* table, const int32_t* cand_kf, int32_t n_candidates,
                                  const int32_t* list_start, const int32_t* point_idx, const uint8_t* own_level, const uint8_t* removed,
                                  int32_t th_obs, int32_t device, int32_t* n_counted, int32_t* n_redundant, uint8_t* cull);
/* The three entries above keep device scratch per device between calls; this frees it (waiting for calls in flight). */
int ydorb_map_release(int32_t device);

/* ------------------------------------------------------------------------------------------
 * Resident map table: the observation table of the three passes above, kept in HBM between calls, changed
 * by deltas and queried with no table upload.  The caller chooses the slots: a map point's slot and a keyframe's slot are its for as
 * long as the caller says (the adapter include/ydorb/mapMirror.hpp keeps pointer -> slot maps with free lists).  The device keeps
 * per point slot a fixed record (where its span lies in the pool, bad, reference keyframe slot and level, position), per keyframe
 * slot the camera centre, and one pool of observations.  A replaced span is appended at the pool's tail and the old one becomes
 * garbage; when an append does not fit, the live spans are repacked in ascending slot order into a fresh arena of the same capacity
 * when live + incoming <= capacity / 2, of 2 x (live + incoming) otherwise (at most INT32_MAX entries).
 * The set_* entries do no device work: they validate and stage.  A slot named several times between two queries is applied once,
 * with its last value.  The next query (or export) uploads one delta, repacks if needed, applies it, and then runs the pass; with
 * nothing staged no table byte moves.  One mutex per handle: LocalMapping may stage while LoopClosing queries.
 * Every malformed input returns YDORB_ERR_INVALID_ARG with the first offender named, before any device work: null arrays, starts
 * that do not begin at 0 or decrease, a negative slot, obs_kf or ref_kf outside 0..n_keyframes-1 (set a new keyframe's centre before
 * points name it), a query slot outside 0..n_points-1, ref_level >= n_levels for a point the query updates, a pool past INT32_MAX
 * entries.  A set_points / set_positions call that fails validation stages nothing.
 * ---------------------------------------------------------------------------------------- */
typedef struct ydorb_mapdb ydorb_mapdb_t;
typedef struct YdMapDbStats {
  int32_t n_points, n_keyframes;        /* 1 + the highest slot named so far (staged changes included) */
  int64_t n_observations;               /* live observations (staged changes included): what ydorb_mapdb_export returns */
  int64_t pool_used, pool_capacity;     /* pool entries used (live + garbage) and allocated, as of the last sync */
  int32_t repacks_kept, repacks_grown;  /* repacks into an arena of the same capacity / of a larger one */
  int32_t point_table_growths, keyframe_table_growths;
  int32_t point_capacity, keyframe_capacity;   /* as of the last sync */
  int64_t last_sync_bytes;              /* what the most recent query (or export) uploaded for the table: 0 when nothing was staged */
  int64_t last_sync_records;            /* ... and its point + position + centre records; the query's own arrays are in neither */
} YdMapDbStats;
/* The capacities are initial (>= 0): every table grows on demand. */
int ydorb_mapdb_create(int32_t device, int32_t point_capacity, int32_t keyframe_capacity, int64_t observation_capacity,
                       ydorb_mapdb_t** out);
void ydorb_mapdb_destroy(ydorb_mapdb_t* db);
/* Map::clear: no points, no keyframes, an empty pool.  Capacities and the repack / growth counters stay. */
int ydorb_mapdb_clear(ydorb_mapdb_t* db);
/* Camera centres of n keyframe slots, centre [n][3].  n_keyframes becomes 1 + the highest slot ever named. */
int ydorb_mapdb_set_centres(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n, const float* centre);
/* Replaces the whole record of each named point: obs_start [n+1] / obs_kf / obs_level = its observers in the container's iteration
 * order (level byte as in YdObservationTable), bad, ref_kf, ref_level [n], pos [n][3].  An empty span with bad = 1 is an erased
 * point.  n_points becomes 1 + the highest slot named; a slot below n_points that was never set reads as bad with no observations. */
int ydorb_mapdb_set_points(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, const int32_t* obs_start, const int32_t* obs_kf,
                           const uint8_t* obs_level, const uint8_t* bad, const int32_t* ref_kf, const uint8_t* ref_level,
                           const float* pos);
/* Positions alone, pos [n][3] (a BA write-back that changes no topology).  The slots must be below n_points. */
int ydorb_mapdb_set_positions(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, const float* pos);
/* ydorb_map_update_normal_depth for the n named points only, results in the order given ([n] and [n][3]); a slot may repeat. */
int ydorb_mapdb_update_normal_depth(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, const float* scale_factors, int32_t n_levels,
                                    float* normal, float* min_distance, float* max_distance, uint8_t* status);
/* ydorb_map_covisibility / ydorb_map_keyframe_redundancy over the resident table: point_idx holds point slots, query_kf / cand_kf /
 * removed [n_keyframes] keyframe slots.  Results, status codes and the capacity rule are those of the flat entries. */
int ydorb_mapdb_covisibility(ydorb_mapdb_t* db, const int32_t* query_kf, int32_t n_queries, const int32_t* list_start,
                             const int32_t* point_idx, const int32_t* out_start, int32_t* conn_kf, int32_t* conn_weight, int32_t* counts,
                             uint8_t* status);
int ydorb_mapdb_keyframe_redundancy(ydorb_mapdb_t* db, const int32_t* cand_kf, int32_t n_candidates, const int32_t* list_start,
                                    const int32_t* point_idx, const uint8_t* own_level, const uint8_t* removed, int32_t th_obs,
                                    int32_t* n_counted, int32_t* n_redundant, uint8_t* cull);
int ydorb_mapdb_stats(ydorb_mapdb_t* db, YdMapDbStats* stats);
/* Reads the device's table back (after applying what is staged) as one flat YdObservationTable plus the four arrays: obs_start
 * [n_points+1], obs_kf / obs_level [n_observations], bad / ref_kf / ref_level [n_points], pos [n_points][3], centre
 * [n_keyframes][3], sized from ydorb_mapdb_stats. */
int ydorb_mapdb_export(ydorb_mapdb_t* db, int32_t* obs_start, int32_t* obs_kf, uint8_t* obs_level, uint8_t* bad, int32_t* ref_kf,
                       uint8_t* ref_level, float* pos, float* centre);

/* Map correction (DESIGN.md section 2 "Map correction", section 6n): the three loops of LoopClosing that move map points through a
 * pair of per-keyframe transforms, run on the resident table in place.  Only per-keyframe tables go up; the new positions (and, when
 * asked for, normals and distances) come back, and the table - device and host mirror - holds them afterwards.  The reference source
 * is absent from this repository; the loops are restated from ORB-SLAM2:
 *   A  LoopClosing::correctLoop: for every keyframe of CorrectedSim3 in the container's order, every map point of
 *      getMapPointMatches() that is not null, not bad and not yet marked mnCorrectedByKF gets
 *      P' = float(correctedSwi.map(Siw.map(double(P)))), setWorldPos, the mark, and updateNormalAndDepth() at once; the keyframe's
 *      own setPose follows its points, so the normals see the new centres of the keyframes before it only.
 *      One call: SIM3 + INTERLEAVED, the entries = the keyframes' lists concatenated, corrector = the list's rank.
 *   B  the tail of Optimizer::optimizeEssentialGraph: all poses are set, then every non-bad point gets
 *      P' = float(correctedSwr.map(Srw.map(double(P)))) with r = mnCorrectedReference where loop A corrected the point, else its
 *      reference keyframe, and updateNormalAndDepth().  One call: SIM3 + POSES_FIRST, slots NULL, corrector = that rank or -1.
 *   C  the map update of LoopClosing::runGlobalBundleAdjust: a point the BA held takes mPosGBA (ydorb_mapdb_set_positions); every
 *      other point whose reference keyframe was reached gets Xc = Rcw_bef P + tcw_bef (mTcwBefGBA), P' = Rwc Xc + twc
 *      (getPoseInverse() after the update) in CV_32F, and no updateNormalAndDepth.  One call: SE3, no normals, -1 correctors with
 *      the reached keyframes in kf_slots (the others come back NOT_COVERED).  The spanning-tree propagation stays with the caller.
 * Assumptions for a maintainer who holds the reference to check: the marks (mnCorrectedByKF, mnCorrectedReference) have no other
 * reader inside the loops; setWorldPos stores the float matrix it is given; the CV_32F products of loop C are OpenCV's gemm (each
 * product exact in double, summed in ascending index with the addend, rounded once); Sim3::map is s * (r * xyz) + t in double;
 * the camera centre after a pose change is what setPose computes (-Rcw^T tcw), which the caller passes as centre_after.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender before any device work, stages nothing and changes
 * nothing: null arrays the mode needs, a point slot outside 0..n_points-1, a keyframe slot outside 0..n_keyframes-1 or repeated, a
 * corrector outside -1..n_kf-1, n != n_points with null slots, a non-positive or non-finite Sim3 scale, n_levels outside 1..8,
 * ref_level >= n_levels for a point whose normals are computed, an unknown arithmetic or centres value, a centres rule without
 * centre_after.
 * ---------------------------------------------------------------------------------------- */
#define YDORB_MAPCORR_SIM3 0          /* before / after: double [n_kf][8], qx qy qz qw tx ty tz s as in YdEssentialGraph::sim3 */
#define YDORB_MAPCORR_SE3 1           /* before / after: float [n_kf][12], a row-major 3x3 followed by the translation */
#define YDORB_MAPCORR_RESIDENT 0      /* every observer shows the centre the table held when the call began */
#define YDORB_MAPCORR_INTERLEAVED 1   /* an observer whose rank in kf_slots is below the correcting keyframe's shows its centre_after */
#define YDORB_MAPCORR_POSES_FIRST 2   /* every keyframe of the call shows its centre_after */
/* status byte of an entry: the first that matches, in this order */
#define YDORB_MAPCORR_BAD 1           /* the resident bad flag is set (a slot never set included): isBad() */
#define YDORB_MAPCORR_CLAIMED 2       /* an earlier entry of this call that was not bad named the slot: mnCorrectedByKF */
#define YDORB_MAPCORR_NOT_COVERED 3   /* corrector -1 and the resident ref_kf is not among kf_slots */
#define YDORB_MAPCORR_DONE 0          /* the position is corrected and, when asked for, the normals are recomputed */
#define YDORB_MAPCORR_DONE_NO_OBSERVATIONS 4   /* corrected; the span is empty, the normals stay zero (the reference's early return) */
typedef struct YdMapCorrection {
  int32_t n_kf;                /* keyframes of the call */
  int32_t arithmetic;          /* YDORB_MAPCORR_SIM3 / _SE3 */
  const int32_t* kf_slots;     /* [n_kf] distinct keyframe slots in the caller's order (loop A: the iteration order of CorrectedSim3) */
  const void* before;          /* SIM3: Siw as it was (g2oSiw / Srw).  SE3: Rcw | tcw of the pose before (mTcwBefGBA) */
  const void* after;           /* SIM3: the corrected Siw (g2oCorrectedSiw); the entry inverts it.  SE3: Rwc | twc of getPoseInverse() after */
  const float* centre_after;   /* [n_kf][3] the camera centres after the correction, or NULL.  When given the table holds them once the
                                  call returns (what setPose leaves in getCameraCenter()) */
  int32_t centres;             /* YDORB_MAPCORR_RESIDENT / _INTERLEAVED / _POSES_FIRST: which centres the normals see */
  int32_t n;                   /* entries */
  const int32_t* slots;        /* [n] point slots; NULL with n == n_points: every slot 0 .. n_points-1 in order */
  const int32_t* corrector;    /* [n] the index into kf_slots of the keyframe that corrects the entry, -1 = the point's resident ref_kf;
                                  NULL: all -1 */
  const float* scale_factors;  /* [n_levels], as in ydorb_mapdb_update_normal_depth; not read when no normals are asked for */
  int32_t n_levels;
  int32_t reserved;            /* 0 */
  float* normal;               /* [n][3] \                                                                         */
  float* min_distance;         /* [n]     > updateNormalAndDepth() with the new position; all three NULL: no normals pass */
  float* max_distance;         /* [n]    /                                                                         */
  float* pos_out;              /* [n][3] the corrected position, the floats the table now holds */
  uint8_t* status;             /* [n] YDORB_MAPCORR_*; an entry that is not DONE* has zero rows and leaves the table alone */
} YdMapCorrection;
/* Applies what is staged, then corrects.  n == 0 still writes the centres.  Holds the handle's mutex. */
int ydorb_mapdb_correct(ydorb_mapdb_t* db, const YdMapCorrection* correction);

/* Keyframe rows (DESIGN.md section 2 "Local map", section 6o): the second relation of the resident table, keyframe -> map points.
 * A row is a keyframe's map-point vector (getMapPointMatches()) as point slots in keypoint order, -1 = a null entry; a keyframe slot
 * whose row was never set has length 0.  The device keeps rowStart / rowLen per keyframe slot and one row pool, under the
 * observation pool's policy (append at the tail, a replaced or erased row becomes garbage, repack in ascending keyframe slot when an
 * append does not fit, same capacity when live + incoming <= capacity / 2, else 2 x (live + incoming), at most INT32_MAX entries).
 * The two setters validate and stage; the next query or export applies rows after points, so a row may name a point staged in the
 * same interval.  A row named several times between two syncs is applied once with its last value; an entry change to a row staged
 * in the same interval lands inside it; entry changes to a resident row are coalesced per (keyframe, index), last value wins.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender, before any device work, and stages nothing: null
 * arrays, a row_start that does not begin at 0 or decreases, a negative keyframe slot, a point slot outside -1..n_points-1 (staged
 * points count: set the point before a row names it), idx outside the row's current length (a staged row's length counts), a row
 * pool past INT32_MAX entries.  Row traffic is accounted in YdMapDbRowStats only; YdMapDbStats keeps its meaning.
 * The two queries restate Tracking::updateLocalPoints / updateLocalKeyFrames of ORB-SLAM2 (the reference source is absent from this
 * repository).  Assumptions for a maintainer who holds the reference to check: updateLocalPoints walks m_v_localKeyFrames in order and
 * each keyframe's getMapPointMatches() in keypoint order, skips null and isBad() points and those already carrying this frame's
 * trackReferenceForFrame mark, and pushes the rest; updateLocalKeyFrames counts, per frame map point that is not bad, every keyframe
 * of getObservations() once (a bad point's frame entry is nulled instead); searchLocalPoints skips the frame's own matches.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdMapDbRowStats {
  int64_t n_entries;                    /* entries of all rows, null ones included (staged changes included): what export_rows returns */
  int64_t pool_used, pool_capacity;     /* row pool entries used (live + garbage) and allocated, as of the last sync */
  int32_t repacks_kept, repacks_grown;
  int32_t header_growths, header_capacity;   /* the rowStart / rowLen tables, as of the last sync */
  int64_t last_row_sync_bytes;          /* what the most recent query (or export) uploaded for the rows: 0 when none was staged */
  int64_t last_row_sync_records;        /* ... and its row header + single entry records */
} YdMapDbRowStats;
/* Replaces the whole row of each named keyframe: row_start [n+1] / point_slot.  A row of length 0 erases it (a culled keyframe).
 * n_keyframes becomes 1 + the highest slot named, as for set_centres (a new slot's centre is zero until set). */
int ydorb_mapdb_set_keyframe_rows(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n, const int32_t* row_start,
                                  const int32_t* point_slot);
/* Single entries: row kf_slot[i], position idx[i] becomes point_slot[i] (addMapPoint, eraseMapPointMatch, replaceMapPointMatch). */
int ydorb_mapdb_set_row_entries(ydorb_mapdb_t* db, const int32_t* kf_slot, const int32_t* idx, const int32_t* point_slot, int32_t n);
/* Reads the device's rows back (after applying what is staged): row_start [n_keyframes+1], point_slot [n_entries]. */
int ydorb_mapdb_export_rows(ydorb_mapdb_t* db, int32_t* row_start, int32_t* point_slot);
int ydorb_mapdb_row_stats(ydorb_mapdb_t* db, YdMapDbRowStats* stats);
/* The points of a keyframe set (updateLocalPoints; the local points of localBundleAdjust).  E = the resident rows of kf_slots
 * concatenated in the order given.  An entry is kept when it is not -1, the point's resident bad flag is clear (a never-set slot reads
 * as bad) and no earlier position of E holds the same slot.  out_slots [count] = the kept entries in the order of E; out_seen[i] = 1
 * when out_slots[i] occurs among seen_points [n_seen] (-1 entries there are ignored; NULL with n_seen = 0).  A keyframe slot may
 * repeat (its second copy keeps nothing); a slot with no row contributes nothing.  capacity >= min(|E|, n_points) always fits; with
 * count > capacity status = 1, out_* are not written and *count is the size needed.  n_kf == 0: count = 0, nothing is applied.
 * Refused up front: null arrays, a keyframe slot outside 0..n_keyframes-1, a seen slot outside -1..n_points-1, negative counts. */
int ydorb_mapdb_points_of_keyframes(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n_kf, const int32_t* seen_points, int32_t n_seen,
                                    int32_t capacity, int32_t* out_slots, uint8_t* out_seen, int32_t* count, uint8_t* status);
/* The observer counter of point lists (updateLocalKeyFrames; the fixed keyframes of localBundleAdjust).  Per list the keyframes with
 * a non-zero count ascending by slot with their counts: ydorb_mapdb_covisibility's result and capacity rule with no own slot
 * excluded.  -1 entries of point_slots are skipped; a point listed twice counts twice; point_bad [list_start[n_lists]] = the resident
 * bad flag of each listed point (0 for a -1 entry). */
int ydorb_mapdb_observer_counter(ydorb_mapdb_t* db, int32_t n_lists, const int32_t* list_start, const int32_t* point_slots,
                                 const int32_t* out_start, int32_t* conn_kf, int32_t* conn_weight, int32_t* counts, uint8_t* status,
                                 uint8_t* point_bad);

/* Local BA graph (DESIGN.md section 2 "Local BA graph on the resident table: the integer contract", section 6u): the flat graph that
 * the adapter's localBundleAdjustImpl (include/ydorb/optimizer.hpp:59-113; the reference's src/optimizer.cpp:140-283) assembles by
 * walking keyframes, map points and observation maps on the host, assembled on the device from what is resident: the keyframe rows,
 * the point views, the keyframe features (ydorb_mapdb_enable_features, declared below), the fp32 positions and the bad flags.  Only the
 * poses are not resident; the caller fills them.  The result is integer selection plus exact fp32 -> fp64 widening, and equals the
 * sequential loops bit for bit, edge order included (the BA's fixed-order sums depend on it).
 *   1. local points   the rows of kf_slots concatenated in the order given; the entries that are not -1, not bad and the first
 *                     occurrence of their slot, in that order: ydorb_mapdb_points_of_keyframes with n_seen = 0.
 *   2. usable         a keyframe is usable (= !isBad()) when it has a feature span of length > 0; a view is usable when its keyframe
 *                     is and idx is below that length.
 *   3. fixed          walk the local points in order and each point's views in span order: a usable keyframe that is not in kf_slots
 *                     is appended at its first occurrence, whatever that view's idx (a view past the feature length still names
 *                     a keyframe that is not bad; such a keyframe may end up with a pose and no edge).
 *   4. edges          the same walk emits one edge per usable view.  Every usable observer is local or fixed, so the reference's
 *                     poseIndex lookup (optimizer.hpp:104-105) never misses and its maxKFid test (:103) is vacuous.  edge_pose = the
 *                     keyframe's index in the pose list, edge_point = the point's rank in the local point list, meas = ((double)kp.x,
 *                     (double)kp.y, right_x < 0 ? -1.0 : (double)right_x), inv_sigma2 = (double)inv_level_sigma2[kp.octave];
 *                     points[p] = the resident fp32 position widened to double.
 *   5. point_status   an OR of the bits below; 0 = every view was usable.  A point without an edge stays in the point list, as in the
 *                     reference.
 * Every keyframe of kf_slots gets a pose, pose i < n_local being kf_slots[i], with pose_fixed = 0: the caller leaves bad keyframes out
 * of the list, as the adapter does, and marks keyframe id 0 as fixed itself.
 * Result memory: the arrays live in pinned host memory owned by the handle and stay valid until the next ydorb_mapdb_local_ba_graph,
 * ydorb_mapdb_clear or destroy on that handle; problem.poses ([n_poses][7], left for the caller) and problem.pose_fixed are writable
 * there.  A caller-capacity protocol like points_of_keyframes' was considered and rejected: the edge count has no cheap bound on the
 * caller's side, and the BA's upload is faster from pinned memory.
 * Refused up front on the host with YDORB_ERR_INVALID_ARG naming the first offender, before any device work and with the handle and
 * the previous result unchanged: null arguments, n_kf < 0, a slot outside 0..n_keyframes-1, a slot repeated in kf_slots, features not
 * enabled.  (The view relation of this handle is always present; MapMirror::localBaGraph of include/ydorb/mapMirror.hpp refuses when
 * enableDescriptors() was not called, because the mirror stages views only then.)
 * n_kf == 0 gives an empty graph, launches nothing and leaves what is staged staged.  Otherwise the call applies what is staged, in
 * the handle's usual order, before it reads, and takes the table's mutex as the other queries do.
 * Assumptions for a maintainer who holds the reference to check: the order of MapPoint::getObservations() is that of the view spans
 * (the caller stages views in that order, as for computeDistinctiveDescriptors); KeyFrame::isBad() <=> the keyframe has no feature
 * span (a culled keyframe's features are erased with a span of length 0); every keyframe observing a local point carries the
 * m_int_localBAForKeyFrameID / m_int_fixedBAForKeyFrameID tags only from this call (optimizer.hpp:61-76). */
#define YDORB_LBA_POINT_SKIPPED_VIEWS 1      /* some view named an unusable keyframe: normal */
#define YDORB_LBA_POINT_VIEW_OUT_OF_RANGE 2  /* a view of a usable keyframe has idx >= the feature length: it emits nothing, nothing is read for it */
#define YDORB_LBA_POINT_NO_EDGES 4           /* the point produced no edge */
typedef struct YdLocalBaGraph {
  YdBaProblem problem;         /* all arrays filled except: poses (allocated [n_poses][7], left for the caller), fx..bf and stop
                                  (caller); pose_fixed = 0 for local, 1 for fixed keyframes */
  int32_t n_local, n_fixed;    /* problem.n_poses = n_local + n_fixed; pose i < n_local is kf_slots[i] */
  const int32_t* pose_kf;      /* [n_poses] keyframe slot of every pose */
  const int32_t* point_slot;   /* [n_points] */
  const int32_t* edge_kf;      /* [n_edges] keyframe slot and */
  const int32_t* edge_idx;     /* [n_edges] keypoint index of every edge: what the write-back erases */
  const uint8_t* point_status; /* [n_points] YDORB_LBA_POINT_* */
} YdLocalBaGraph;
typedef struct YdMapDbLbaStats {
  int64_t n_calls;                      /* calls that passed validation */
  int64_t last_launches, last_syncs;    /* kernels launched (the staged deltas' not counted) and stream synchronisations of the last call */
  int64_t last_upload_bytes, last_download_bytes;   /* the call's own arrays up; the counts and the result down */
  int64_t last_n_local, last_n_fixed, last_n_points, last_n_edges;
  /* device time of the last call's phases from event pairs, filled only after ydorb_mapdb_lba_set_profiling(db, 1), else 0:
   * the local points (k_rowset_*), the view walk (rank, mark, count, scan), the emit (fixed, edges, reset), the result's read-back */
  double last_ms_points, last_ms_walk, last_ms_emit, last_ms_copy;
} YdMapDbLbaStats;
int ydorb_mapdb_local_ba_graph(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n_kf, const float* inv_level_sigma2 /*[8]*/,
                               YdLocalBaGraph* out);
int ydorb_mapdb_lba_stats(ydorb_mapdb_t* db, YdMapDbLbaStats* stats);
/* Opt-in: six stream events round the phases of every later call (a few microseconds of stream time each); off by default. */
int ydorb_mapdb_lba_set_profiling(ydorb_mapdb_t* db, int32_t on);

/* Resident descriptors (DESIGN.md section 2 "Distinctive descriptor on the resident table", section 6p): two more relations of the
 * resident table and the query that closes the pair computeDistinctiveDescriptors() / updateNormalAndDepth() on it.
 *   blocks  keyframe slot -> the keyframe's descriptor matrix [n_k][32] in keypoint order (m_cvMat_descriptors).  A keyframe's
 *           descriptors never change after it is made: a block goes up once.  A block of length 0 erases it: a culled keyframe, the
 *           reference's pKF->isBad().  The pool is counted in descriptors of 32 bytes.
 *   views   point slot -> where the point is seen, (keyframe slot, keypoint index) pairs in the order computeDistinctiveDescriptors
 *           iterates getObservations() in: the order of obs_kf in ydorb_mapdb_set_points.  They are stored apart from the observation
 *           pool, whose layout, records and YdMapDbStats keep their meaning.
 * Both lie in pools under the observation pool's policy (append at the tail, a replaced or erased span becomes garbage, repack in
 * ascending slot order when an append does not fit, same capacity when live + incoming <= capacity / 2, else 2 x (live + incoming), at
 * most INT32_MAX entries; a view counts as two entries there).  The pools start empty-handed and grow on demand;
 * ydorb_mapdb_reserve_descriptors sizes them, and is refused unless both are empty (before the first setter, or after clear).
 * The two setters validate and stage and do no device work; the next query or export applies them after points and rows, so a view may
 * name a keyframe, and a query a point, staged in the same interval.  A slot named several times between two syncs is applied once,
 * with its last value.  With nothing staged for the two relations a sync launches nothing for them and moves no byte.  Their traffic
 * is accounted in YdMapDbDescStats only.  set_keyframe_descriptors grows n_keyframes as set_keyframe_rows does.  ydorb_mapdb_clear
 * empties both and keeps capacities and counters.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender, before any device work, and stages nothing: null
 * arrays, a start array that does not begin at 0 or decreases, a negative slot, a view's point slot outside 0..n_points-1 (set the
 * point before its views), view_kf outside 0..n_keyframes-1 (staged slots count),
 * a negative view_idx, a view span longer than 65535, a pool past INT32_MAX entries, a query slot outside 0..n_points-1, null outputs
 * with n > 0.  A view_idx at or past its keyframe's block length cannot be refused when staged (the block may come later, or change):
 * the query finds it on the device and reports it per point as a status, in no error.
 * The query restates MapPoint::computeDistinctiveDescriptors of ORB-SLAM2 (the reference source is absent from this repository) on the
 * rule of ydorb_distinctive_descriptors above: the median is (int)(0.5 m) of the sorted distance row, the first row with the least
 * median wins.  Assumptions for a maintainer who holds the reference to check: the function returns first for a bad point; it walks
 * getObservations() in the container's order, skips observations whose keyframe isBad() and collects
 * pKF->m_cvMat_descriptors.row(idx) of the others; it returns without a change when nothing was collected; m is the number of
 * collected rows; m_descriptor becomes a copy of the winning row.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdMapDbDescStats {
  int64_t n_views, n_descriptors;               /* live, staged changes included */
  int64_t view_pool_used, view_pool_capacity;   /* as of the last sync, in views */
  int64_t desc_pool_used, desc_pool_capacity;   /* ... in descriptors */
  int32_t view_repacks_kept, view_repacks_grown, desc_repacks_kept, desc_repacks_grown;
  int64_t last_desc_sync_bytes, last_desc_sync_records;   /* 0 when nothing of these two relations was staged */
} YdMapDbDescStats;
/* status byte of a queried point: the first that matches, in this order */
#define YDORB_MAPDESC_BAD 1                 /* the resident bad flag is set (a slot never set included): the reference returns first */
#define YDORB_MAPDESC_NO_DESCRIPTORS 2      /* after skipping views whose keyframe holds no block nothing is left */
#define YDORB_MAPDESC_VIEW_OUT_OF_RANGE 3   /* a view of a keyframe with a block has idx >= the block's length; no descriptor was read */
#define YDORB_MAPDESC_UPDATED 0             /* the winner was computed */
/* Initial capacities of the view pool (in views) and of the descriptor pool (in descriptors); both pools must be empty. */
int ydorb_mapdb_reserve_descriptors(ydorb_mapdb_t* db, int64_t view_capacity, int64_t descriptor_capacity);
/* Replaces the whole block of each named keyframe: desc_start [n+1] / desc [desc_start[n]][32].  A block of length 0 erases it. */
int ydorb_mapdb_set_keyframe_descriptors(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n, const int32_t* desc_start,
                                         const uint8_t* desc);
/* Replaces the views of each named point: view_start [n+1] / view_kf / view_idx [view_start[n]].  An empty span erases them. */
int ydorb_mapdb_set_point_views(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, const int32_t* view_start, const int32_t* view_kf,
                                const int32_t* view_idx);
/* computeDistinctiveDescriptors() of the n named points with no descriptor upload; a slot may repeat, results in the order given.
 * status [n] = YDORB_MAPDESC_*.  For an UPDATED point best = the position of the winning view within the point's view span (skipped
 * views counted, so the caller can index its own list with it), best_view [n][2] = that view's (keyframe slot, keypoint index),
 * desc_out [n][32] = the winning row.  Every other status: best = -1 and zero rows; the call still returns YDORB_OK. */
int ydorb_mapdb_distinctive_descriptors(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, int32_t* best, int32_t* best_view,
                                        uint8_t* desc_out, uint8_t* status);
/* Reads the device's views back (after applying what is staged): view_start [n_points+1], view_kf / view_idx [n_views]. */
int ydorb_mapdb_export_views(ydorb_mapdb_t* db, int32_t* view_start, int32_t* view_kf, int32_t* view_idx);
/* ... and its blocks: desc_start [n_keyframes+1], desc [n_descriptors][32]. */
int ydorb_mapdb_export_descriptors(ydorb_mapdb_t* db, int32_t* desc_start, uint8_t* desc);
int ydorb_mapdb_desc_stats(ydorb_mapdb_t* db, YdMapDbDescStats* stats);

/* Resident point attributes (DESIGN.md section 2 "Local map on the resident table", section 6q): what Tracking::searchLocalPoints
 * reads of a map point besides its position, kept where the resident queries compute it.  Per point slot: normal [3], the raw
 * minDistance / maxDistance of updateNormalAndDepth (not the 0.8 / 1.2 multiples), desc [32] and a flag byte (bit 0: the geometry
 * group normal + distances is set, bit 1: the descriptor is set).  The relation is opt-in: a handle that never calls
 * ydorb_mapdb_enable_attributes allocates nothing for it, launches nothing for it and every entry below but enable and attr_stats
 * returns YDORB_ERR_INVALID_ARG.  YdMapDbStats, YdMapDbRowStats and YdMapDbDescStats keep their meaning either way.
 * The arrays lie in an arena of their own that covers the point table's capacity and grows with it (device-to-device copy, new slots
 * zero).  set_point_attributes validates and stages and does no device work; the next query or export applies the delta after points,
 * rows, views and blocks.  A slot named several times between two syncs yields one record, each group with its last value.
 * ydorb_mapdb_set_points of a point with bad = 1 and an empty span (an erased point) stages a clear of that slot: flags 0 and all-zero
 * values, what a slot never set reads as; attributes staged for the slot before the erase are dropped, those staged after it stay.
 * ydorb_mapdb_clear zeroes the arrays and keeps capacity and counters.
 * Write-through: with attributes enabled, ydorb_mapdb_update_normal_depth leaves normal and distances of every entry it computed
 * (status 0) in the arrays and sets bit 0; ydorb_mapdb_correct does the same for the entries that end YDORB_MAPCORR_DONE in a call
 * that asked for normals (DONE_NO_OBSERVATIONS, CLAIMED, BAD, NOT_COVERED and a call without a normals pass write nothing);
 * ydorb_mapdb_distinctive_descriptors leaves the winning row of every YDORB_MAPDESC_UPDATED entry and sets bit 1.  The copy runs on the
 * device behind the query, from its result buffer; attributes staged before the query are applied by the query's sync and so lose
 * to it.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender, before any device work, and stages nothing. */
typedef struct YdMapDbAttrStats {
  int32_t enabled, growths;                 /* growths: of the attribute arena, with the point table */
  int64_t capacity;                         /* point slots the arena covers as of the last sync; 0 when not enabled */
  int64_t last_attr_sync_bytes, last_attr_sync_records;   /* 0 when nothing of this relation was staged */
  int64_t last_write_through_records;       /* entries the last of the three write-through queries left in the arrays */
} YdMapDbAttrStats;
/* Turns the relation on; calling it twice is fine. */
int ydorb_mapdb_enable_attributes(ydorb_mapdb_t* db);
/* Stages attributes of the n named slots: normal [n][3], min_distance [n], max_distance [n] (all three or none) and desc [n][32] may
 * each be NULL; a NULL group leaves that group and its flag alone.  Refused: null slots with n > 0, both groups NULL, a partial
 * geometry group, a slot outside 0..n_points-1 (staged points count). */
int ydorb_mapdb_set_point_attributes(ydorb_mapdb_t* db, const int32_t* slots, int32_t n, const float* normal, const float* min_distance,
                                     const float* max_distance, const uint8_t* desc);
/* Applies what is staged, then reads back: normal [n_points][3], min_distance / max_distance / flags [n_points], desc [n_points][32]. */
int ydorb_mapdb_export_attributes(ydorb_mapdb_t* db, float* normal, float* min_distance, float* max_distance, uint8_t* desc,
                                  uint8_t* flags);
int ydorb_mapdb_attr_stats(ydorb_mapdb_t* db, YdMapDbAttrStats* stats);

/* Tracking::searchLocalPoints on the resident table (DESIGN.md section 2 "Local map on the resident table"): the frustum test and the
 * fused search read each listed point by slot and no map value travels up.  Row i of the table the flat entries would be given is
 *   pos_min    = (resident position, 0.8f * minDistance)      one fp32 multiply: the bits getMinDistanceInvariance() returns
 *   normal_max = (resident normal,   1.2f * maxDistance)      ... getMaxDistanceInvariance()
 *   max_distance = the raw maxDistance, desc = the resident descriptor
 * of point_slots[i]; has_observations = the resident observation span is not empty; the effective skip = the caller's skip byte OR
 * the resident bad flag (a slot never set included). */
#define YDORB_FRUSTUM_NO_ATTRIBUTES 7 /* listed, not skipped, and the geometry flag (fused search: or the descriptor flag) is not set:
                                         treated as not in view, zero track row, query flags 0 */
/* ydorb_frustum_cull over the resident values: views [n_views], list_start [n_views+1], point_slots / skip / rows / status
 * [list_start[n_views]], n_in_view [n_views] or NULL.  Runs on the handle's own stream. */
int ydorb_mapdb_frustum_cull(ydorb_mapdb_t* db, const YdFrustumView* views, int32_t n_views, const int32_t* list_start,
                             const int32_t* point_slots, const uint8_t* skip, YdTrackView* rows, uint8_t* status, int32_t* n_in_view);
/* ydorb_search_local_points with the table above; the query descriptors are copied on the device and never exist on the host.
 * assigned[idx] = the list index i, not the slot.  A slot may repeat and then behaves as the flat entry does with equal rows.  Refused
 * up front: null arguments, n < 0, a slot outside 0..n_points-1, n_levels outside 1..8, an invalid frame view, attributes not
 * enabled, db and m on different devices.  n == 0 returns YDORB_OK with zero counts and launches nothing. */
int ydorb_mapdb_search_local_points(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdFrameView* frame, const YdFrustumView* view,
                                    const int32_t* point_slots, int32_t n, const uint8_t* skip, float th, float ratio, uint8_t* taken,
                                    int32_t* assigned, YdTrackView* rows, uint8_t* status, int32_t* n_to_match, int32_t* n_matches);

/* Resident keyframe features (DESIGN.md section 2 "Fuse search on the resident table", section 6r): one more relation of the resident
 * table and the query that runs the search of LocalMapping::searchInNeighbors / LoopClosing::searchAndFuse for all targets at once.
 *   features  keyframe slot -> the keyframe's undistorted keypoints [n_k] (m_v_keyPoints) and right_x [n_k] (m_v_rightXcords), in
 *             keypoint order: the order and the n_k of the keyframe's descriptor block.  A keyframe's features never change after
 *             it is made: they go up once.  A span of length 0 erases them.  The pool is counted in features; one span per keyframe
 *             indexes two device arrays, KeyPoint [n_k] and float [n_k], each contiguous.
 * The relation is opt-in: a handle that never calls ydorb_mapdb_enable_features allocates nothing for it, launches nothing for it and
 * every entry below but enable and feat_stats returns YDORB_ERR_INVALID_ARG.  YdMapDbStats, YdMapDbRowStats, YdMapDbDescStats and
 * YdMapDbAttrStats keep their values either way.  The pool follows the observation pool's policy (append at the tail, a replaced or
 * erased span becomes garbage, repack in ascending slot order when an append does not fit, same capacity when live + incoming <=
 * capacity / 2, else 2 x (live + incoming), at most INT32_MAX features); it starts empty-handed and grows on demand.
 * set_keyframe_features validates and stages and does no device work; the next query or export applies the delta after points, rows,
 * views and blocks and before the attributes.  A slot named several times between two syncs is applied once, with its last value.
 * It grows n_keyframes as set_keyframe_rows does.  ydorb_mapdb_clear empties the relation and keeps capacities and counters.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender, before any device work, and stages nothing: null
 * arrays, a start array that does not begin at 0 or decreases, a negative slot, a span longer than 65535, an octave outside 0..7, a
 * pool past INT32_MAX features.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdMapDbFeatStats {
  int32_t enabled;
  int32_t repacks_kept, repacks_grown;
  int64_t n_features;                           /* live, staged changes included */
  int64_t pool_used, pool_capacity;             /* as of the last sync, in features */
  int64_t last_feat_sync_bytes, last_feat_sync_records;   /* 0 when nothing of this relation was staged */
} YdMapDbFeatStats;
/* Turns the relation on; calling it twice is fine. */
int ydorb_mapdb_enable_features(ydorb_mapdb_t* db);
/* Replaces the features of each named keyframe: feat_start [n+1], kps [feat_start[n]], right_x [feat_start[n]] or NULL (every entry
 * is then stored as -1.0f: a monocular keyframe).  A span of length 0 erases them. */
int ydorb_mapdb_set_keyframe_features(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n, const int32_t* feat_start,
                                      const YdKeyPoint* kps, const float* right_x);
/* Reads the device's features back (after applying what is staged): feat_start [n_keyframes+1], kps / right_x [n_features]. */
int ydorb_mapdb_export_features(ydorb_mapdb_t* db, int32_t* feat_start, YdKeyPoint* kps, float* right_x);
int ydorb_mapdb_feat_stats(ydorb_mapdb_t* db, YdMapDbFeatStats* stats);

/* OrbMatcher::fuseByProjection / fuseBySim3 for several target keyframes in one call (DESIGN.md section 2 "Fuse search on the resident
 * table" fixes the fp32 operation order): per (target, listed point) the predicates of pass 1 on the resident position, normal and
 * raw distances, then the window search of ydorb_fuse_search / ydorb_window_search on the target's resident features and descriptor
 * block with the point's resident descriptor.  What travels up is the targets, the list starts, the slots and the skip bytes. */
typedef struct YdFuseTarget {
  int32_t kf_slot;          /* the target keyframe: its features and its descriptor block are read by slot */
  YdFrustumView view;       /* Rcw, tcw, Ow, intrinsics, bounds, n_levels, level_ratio, scale_factors (viewing_cos_limit unused) */
  float inv_sigma2[8];      /* m_v_invScaleFactorSquares; all zero disables the chi-square test (fuseBySim3) */
  float th;
  int32_t max_dist;         /* 50 for both fuse forms */
  int32_t flags;            /* bit 0: skip a point the target already observes (isInKeyFrame, fuseByProjection);
                               bit 1: ignore right_x, every feature takes the monocular branch (fuseBySim3) */
} YdFuseTarget;
#define YDORB_FUSE_SKIP_OBSERVED 1
#define YDORB_FUSE_MONOCULAR 2
/* status byte of a list entry: the first rule that fires, in this order; every status but 0 searches nothing (best_idx -1) */
#define YDORB_FUSE_SEARCHED 0       /* every predicate held: the window was searched */
#define YDORB_FUSE_SKIPPED 1        /* the caller's skip byte */
#define YDORB_FUSE_BAD 2            /* the resident bad flag is set (a slot never set included) */
#define YDORB_FUSE_OBSERVED 3       /* flag bit 0 and the point's resident observation span holds kf_slot */
#define YDORB_FUSE_NO_ATTRIBUTES 4  /* the geometry flag or the descriptor flag of the attribute record is unset */
#define YDORB_FUSE_REJECTED 5       /* zc >= 0, inside the image (half open), distance range and viewing angle: one does not hold; a NaN is rejected */
/* target_status */
#define YDORB_FUSE_TARGET_OK 0
#define YDORB_FUSE_TARGET_NO_FEATURES 1      /* the keyframe has no feature span */
#define YDORB_FUSE_TARGET_NO_BLOCK 2         /* ... no descriptor block */
#define YDORB_FUSE_TARGET_LENGTH_MISMATCH 3  /* the two lengths differ */
/* targets [n_targets], list_start [n_targets+1]; with L = list_start[n_targets]: point_slots / skip / best_idx / status [L]; n_found
 * and target_status [n_targets].  Target t tests the points point_slots[list_start[t] .. list_start[t+1]).  best_idx[e] = the
 * feature of the target the point matched, or -1; n_found[t] = the matches of target t.  A target with a non-zero target_status has
 * all best_idx -1 and n_found 0 (its status bytes are the predicates' as usual, nothing is searched); the call still returns YDORB_OK.  A slot may repeat within a
 * list and across lists.  The call is synchronous and exact: when the candidate records overflow their pool it grows and the search
 * is replayed.  Refused up front: null arguments, a malformed list_start, a point slot outside 0..n_points-1, a kf_slot outside
 * 0..n_keyframes-1, n_levels outside 1..8, max_dist outside 0..256, attributes or features not enabled, db and m on different
 * devices.  L == 0 launches nothing. */
int ydorb_mapdb_fuse_search(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdFuseTarget* targets, int32_t n_targets,
                            const int32_t* list_start, const int32_t* point_slots, const uint8_t* skip, int32_t* best_idx,
                            uint8_t* status, int32_t* n_found, uint8_t* target_status);

/* Resident BoW feature vectors: a fifth span relation of the resident table.
 *   bow  keyframe slot -> the keyframe's DBoW3::FeatureVector flattened in map order: nodes ascending, and within a node the
 *        features in the vector's order.  The element is the pair (node id, feature index).  A keyframe's feature vector never
 *        changes after it is made: it goes up once.  A span of length 0 erases it.  The pool is counted in entries.
 * The relation is opt-in: a handle that never calls ydorb_mapdb_enable_bow allocates nothing for it, launches nothing for it and
 * every entry below but enable and bow_stats returns YDORB_ERR_INVALID_ARG.  Every other stats struct keeps its values either way.
 * The pool follows the observation pool's policy, as the feature pool does.  set_keyframe_bow validates and stages and does no device
 * work; the next query or export applies the delta after the features and before the attributes.  A slot named several times between
 * two syncs is applied once, with its last value.  It grows n_keyframes as set_keyframe_rows does.  ydorb_mapdb_clear empties the
 * relation and keeps capacities and counters.
 * Every malformed input returns YDORB_ERR_INVALID_ARG naming the first offender, before any device work, and stages nothing: null
 * arrays, a start array that does not begin at 0 or decreases, a negative slot, a span longer than 65535, node ids that decrease
 * inside a span, a node id of 2^31 or more, a feature index outside 0..65534, a feature index that repeats inside one span (DBoW3
 * files each descriptor under one node), a pool past INT32_MAX entries.
 * ---------------------------------------------------------------------------------------- */
typedef struct YdMapDbBowStats {
  int32_t enabled;
  int32_t repacks_kept, repacks_grown;
  int64_t n_entries;                            /* live, staged changes included */
  int64_t pool_used, pool_capacity;             /* as of the last sync, in entries */
  int64_t last_bow_sync_bytes, last_bow_sync_records;   /* 0 when nothing of this relation was staged */
} YdMapDbBowStats;
/* Turns the relation on; calling it twice is fine. */
int ydorb_mapdb_enable_bow(ydorb_mapdb_t* db);
/* Replaces the feature vector of each named keyframe: bow_start [n+1], node_id / feat [bow_start[n]].  node_id is DBoW3's NodeId
 * (unsigned int).  A span of length 0 erases. */
int ydorb_mapdb_set_keyframe_bow(ydorb_mapdb_t* db, const int32_t* kf_slots, int32_t n, const int32_t* bow_start, const uint32_t* node_id,
                                 const int32_t* feat);
/* Reads the device's feature vectors back (after applying what is staged): bow_start [n_keyframes+1], node_id / feat [n_entries]. */
int ydorb_mapdb_export_bow(ydorb_mapdb_t* db, int32_t* bow_start, uint32_t* node_id, int32_t* feat);
int ydorb_mapdb_bow_stats(ydorb_mapdb_t* db, YdMapDbBowStats* stats);

/* LocalMapping::createNewMapPoints over all neighbours in one call (DESIGN.md section 2 "createNewMapPoints on the resident table",
 * section 6t): for neighbour i in the caller's order, OrbMatcher::searchForTriangulation(first, second_i) as
 * ydorb_search_for_triangulation computes it, then the geometry of ydorb_triangulate_matches on its matches, on the table as of the
 * call (staged deltas applied first).  "Has a map point" is "the keyframe's row entry is >= 0" on both sides; for the first keyframe
 * it also covers every idx1 whose match with a neighbour j < i was accepted (status low nibble YDORB_TRI_ACCEPTED): an accepted
 * match claims its idx1 for all later neighbours, as the reference's addMapPoint does.  Keypoints, right_x, descriptors, rows and
 * feature vectors are read by slot; what travels up is the views and one depth array per keyframe. */
typedef struct YdCreateView {   /* one keyframe: YdTriView's constants, with the slot in place of the keypoint pointers */
  int32_t kf_slot;
  int32_t n;                    /* the length of depth */
  const float* depth;           /* host [n] m_v_depth */
  float Tcw[12], Rwc[9], Ow[3];
  float fx, fy, cx, cy, invfx, invfy, b, bf;
  float level_sigma2[8];        /* m_v_scaleFactorSquares, [n_levels] used */
  float scale_factors[8];       /* m_v_scaleFactors, [n_levels] used */
  int32_t n_levels;             /* 1..8 */
} YdCreateView;
typedef struct YdCreateNeighbour {
  YdCreateView view;
  float F[9];                   /* F12 row-major, as ydorb_search_for_triangulation takes it */
  float ex, ey;                 /* the epipole of the first keyframe in the second */
  float ratio_factor;           /* 1.5f * the first keyframe's scale factor */
} YdCreateNeighbour;
#define YDORB_TRI_UNMATCHED 15  /* status low nibble of a feature the neighbour's search did not match */
/* neighbour_status */
#define YDORB_CREATE_NB_OK 0
#define YDORB_CREATE_NB_NO_FEATURES 1      /* the keyframe has no feature span */
#define YDORB_CREATE_NB_NO_BLOCK 2         /* ... no descriptor block */
#define YDORB_CREATE_NB_NO_BOW 3           /* ... no BoW feature vector */
#define YDORB_CREATE_NB_LENGTH_MISMATCH 4  /* features, descriptor block, row and depth differ in length */
#define YDORB_CREATE_NB_BOW_INDEX 5        /* a feature index of the BoW feature vector is not below the feature count */
/* first, neighbours [n_nb]; with n = first->n: matched_second / status [n_nb][n], x3d [n_nb][n][3]; n_matches, n_accepted and
 * neighbour_status [n_nb].  The outputs are dense over the first keyframe's features, so a caller walks a neighbour's matches in
 * ascending idx1 as the reference walks its pair vector: matched_second[i][idx1] = the feature of neighbour i matched to idx1, or -1;
 * x3d / status = ydorb_triangulate_matches' point and byte of that match, 0 0 0 and YDORB_TRI_UNMATCHED where there is none.
 * n_matches[i] = the matches of neighbour i, n_accepted[i] = those accepted.  An unusable neighbour gets a non-zero neighbour_status,
 * searches nothing and has no matches; when the first keyframe is unusable every neighbour gets the first keyframe's status.  The
 * call still returns YDORB_OK.  The results of neighbour i do not depend on any later neighbour, so a caller that makes the
 * reference's abort check between neighbours and stops after neighbour k drops the tail unread.  The call is synchronous and exact:
 * the candidate records start at 16384 per neighbour; when they overflow, the pool grows to what the search asked for and the whole
 * call is replayed, claims reset.
 * Refused up front: null arguments, n_levels outside 1..8, a kf_slot outside 0..n_keyframes-1, first->n not equal to the first
 * keyframe's resident feature count, a second keyframe equal to the first, a second keyframe named twice (the claim rule is the
 * reference's only when each occurs once), features or BoW feature vectors not enabled, db and m on different devices.  n_nb == 0
 * launches nothing. */
int ydorb_mapdb_create_new_points(ydorb_mapdb_t* db, ydorb_matcher_t* m, const YdCreateView* first, const YdCreateNeighbour* neighbours,
                                  int32_t n_nb, int32_t stereo_only, int32_t check_orientation, int32_t* matched_second, float* x3d,
                                  uint8_t* status, int32_t* n_matches, int32_t* n_accepted, uint8_t* neighbour_status);

/* The BoW searches over all candidate keyframes in one call (DESIGN.md section 2 "BoW searches on the resident table", section 6v), on
 * the table as of the call: staged deltas are applied first, in the order ydorb_mapdb_create_new_points applies them.
 * ydorb_mapdb_search_by_bow_keyframes is OrbMatcher::searchByBowInTwoKeyFrames(first, second_i) for every i < n_second
 * (LoopClosing::computeSim3), ydorb_mapdb_search_by_bow_frame is OrbMatcher::searchByBowInKeyFrameAndFrame(kf_i, frame) for every
 * i < n_kf (Tracking::relocalize; n_kf == 1: trackReferenceKeyFrame).  Each pair answers as ydorb_search_by_bow (mode 4 / mode 3) does
 * on the keyframes' resident keypoints, descriptor blocks and feature vectors, with "has a good map point" decided on the device in
 * place of `valid` for every resident side: the keyframe's row entry p is >= 0, below the point table's capacity, and the resident
 * bad flag of p is clear (a slot never set reads as bad: the rule of YDORB_FUSE_BAD).  The frame keeps YdBowSide.valid as the flat
 * call reads it, NULL = every feature.
 * Outputs.  matched_second[i][idx1] (keyframes) / matched_kf_feature[i][idxF] (frame) = the flat call's out[] of pair i, -1 where
 * there is no match.  matched_point = the point slot the reference's match vector would hold, i.e. the row entry of the second
 * keyframe (keyframes) or of the keyframe (frame) at the matched feature, -1 with no match.  n_matches[i] = the reference's return
 * value, histogram culls subtracted.  pair_status[i] = a YDORB_BOW_PAIR_*: an unusable keyframe searches nothing, its outputs are all
 * -1 and its count 0, and the call still returns YDORB_OK; an unusable first keyframe gives every pair its status.
 * The pairs are independent of each other: each has match flags of its own.  So, unlike ydorb_mapdb_create_new_points, whose
 * neighbours claim features from each other, a keyframe may be named several times and a second keyframe may equal the first;
 * repeats answer alike.
 * Refused up front, before any device work, with the first offender named and nothing changed (no staged delta is applied, no
 * counter moves): null arguments, negative counts, a slot outside 0..n_keyframes-1, n_first not equal to the first keyframe's
 * resident feature count, features or BoW feature vectors not enabled (rows and descriptor blocks are not opt-in), db and m on
 * different devices, a ratio that is not finite; for the frame: n outside 0..65535 (a candidate record packs its index in 16 bits),
 * null kps / desc with n > 0, a malformed feature vector (node_start not starting at 0 or decreasing, node ids not strictly
 * ascending, a feature index outside 0..n-1).  These return YDORB_ERR_INVALID_ARG.  More than 65535 pairs in one call (n_second or
 * n_kf: the pairs are one dimension of the launch grid) are refused in the same way with YDORB_ERR_UNSUPPORTED.  n_second == 0 or
 * n_kf == 0 launches nothing and synchronises nothing.
 * The call is synchronous and exact: the candidate records start at 16384 per pair (the pool ydorb_mapdb_create_new_points uses, and
 * the same counter); when they overflow, the pool grows to what the gather asked for and the whole call is replayed.  Four launches,
 * one upload, one read-back and one synchronisation of the matcher's stream per attempt, whatever the number of pairs. */
#define YDORB_BOW_PAIR_OK 0
#define YDORB_BOW_PAIR_NO_FEATURES 1      /* the keyframe has no feature span */
#define YDORB_BOW_PAIR_NO_BLOCK 2         /* ... no descriptor block */
#define YDORB_BOW_PAIR_NO_BOW 3           /* ... no BoW feature vector */
#define YDORB_BOW_PAIR_LENGTH_MISMATCH 4  /* features, descriptor block and row differ in length */
#define YDORB_BOW_PAIR_BOW_INDEX 5        /* a feature index of the BoW feature vector is not below the feature count */
/* second_kf_slots [n_second]; matched_second / matched_point [n_second][n_first]; n_matches / pair_status [n_second] */
int ydorb_mapdb_search_by_bow_keyframes(ydorb_mapdb_t* db, ydorb_matcher_t* m, int32_t first_kf_slot, const int32_t* second_kf_slots,
                                        int32_t n_second, float ratio, int32_t check_orientation, int32_t n_first,
                                        int32_t* matched_second, int32_t* matched_point, int32_t* n_matches, uint8_t* pair_status);
/* kf_slots [n_kf]; matched_kf_feature / matched_point [n_kf][frame->n]; n_matches / pair_status [n_kf] */
int ydorb_mapdb_search_by_bow_frame(ydorb_mapdb_t* db, ydorb_matcher_t* m, const int32_t* kf_slots, int32_t n_kf, const YdBowSide* frame,
                                    float ratio, int32_t check_orientation, int32_t* matched_kf_feature, int32_t* matched_point,
                                    int32_t* n_matches, uint8_t* pair_status);
/* What the two entries above did on this matcher.  launches counts kernel launches (the memsets that clear the outputs are not
 * kernels of this library), a replay after an overflow adds its attempt to attempts, launches, synchronisations and bytes_down.  With
 * profiling on (ydorb_matcher_set_profiling), ms [3] = average device ms per profiled call of the join and gather, of the resolve
 * and of the emit; all zero otherwise. */
typedef struct YdBowSearchStats {
  int64_t calls, attempts;                /* since the matcher was created; calls that reached the device only */
  int64_t launches, synchronisations;     /* of the last such call, over its attempts */
  int64_t bytes_up, bytes_down;           /* of the last such call */
  int64_t pool_per_pair;                  /* candidate records each pair's part of the pool holds now */
  int32_t profiled_calls;
  float ms[3];
} YdBowSearchStats;
int ydorb_matcher_bow_search_stats(ydorb_matcher_t* m, YdBowSearchStats* stats);

#ifdef __cplusplus
}
#endif
#endif /* YDORB_C_API_H */
