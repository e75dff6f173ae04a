/* ============================================================================
 * orbslam_hip.h -- C ABI of the MI355X (gfx950) ORB front-end and bundle-adjustment
 * back-end.  This is the drop-in boundary: the reference has no plugin/FFI layer,
 * its hot path is three C++ classes called directly, so each entry point below
 * names the reference member it replaces (file:line relative to the reference
 * tree).  C++ shims with the reference's own class names and signatures live in
 * ceres_mono_orb_slam2_amd/csrc/compat/ and call nothing but these functions.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ORBHIP_E* code on error;
 *     orbhip_last_error() gives a message for the calling thread's last failure;
 *   - the caller owns every buffer; handles are not thread-safe, distinct handles
 *     are; `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *   - "_device" entry points take device pointers and only ENQUEUE work on
 *     `stream` (no host synchronisation); the others take host pointers and return
 *     after the result is in host memory;
 *   - there is no CPU fallback: without a HIP device every compute entry point
 *     fails with ORBHIP_ENODEV.
 * ========================================================================== */
#ifndef ORBSLAM_HIP_H
#define ORBSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBHIP_OK 0
#define ORBHIP_EINVAL (-1)    /* bad argument */
#define ORBHIP_ENODEV (-2)    /* no HIP device / HIP runtime error */
#define ORBHIP_ENOMEM (-3)
#define ORBHIP_ECAP (-4)      /* caller's output capacity too small */
#define ORBHIP_EOVERFLOW (-5) /* internal candidate capacity exceeded (cannot happen for images up to 4095 x 4095: the candidate arrays
                                 are sized for the worst case; only the ORBHIP_KEYCAP test hook lowers them) */
#define ORBHIP_ENUMERIC (-6)  /* linear solve failed */
#define ORBHIP_ETIMEOUT (-7)  /* a workgroup of a persistent (flag-linked) kernel waited longer than its time limit for another
                                 one: the device is oversubscribed or hung.  Never reported as a numerical failure: the solve
                                 ends with ba_summary.termination 7 and the outputs hold the last accepted iterate */

const char* orbhip_last_error(void);
int orbhip_device_count(void);
/* library version / build tag */
const char* orbhip_version(void);
/* HIP device used by the entry points that take no handle (matcher host-pointer calls, all ba_* calls);
 * default 0.  hipSetDevice is per host thread, so every such call re-selects this device itself. */
int orbhip_set_default_device(int device);
/* The reference runs Tracking, LocalMapping and the loop closer's GlobalBundleAdjustemnt on three threads that here share ONE GPU
 * (src/LocalMapping.cc:89, src/LoopClosing.cc:590,656).  Every host thread has its own HIP stream; a thread that calls this with
 * high != 0 - the Tracking thread - gets the device's greatest stream priority for the calls it makes from then on (its short
 * per-frame kernels are dispatched ahead of another thread's queued bundle-adjustment work).  Results do not depend on it.   */
int orbhip_set_thread_priority(int high);
int orbhip_get_default_device(void);
/* Copy between PINNED host memory (hipHostMalloc / hipHostRegister: mapped into the device's address space) and device memory by a
 * KERNEL on `stream` - the way the library's own host-pointer entry points move their staging blocks.  For callers that feed
 * orbx_extract_batch_device from host frames (src/Frame.cc:116 hands operator() a host cv::Mat): upload, extract + match and download
 * of consecutive batches then overlap as ordinary concurrent kernels on three streams, without the runtime's copy-engine path
 * (which stalls host threads that copy concurrently, and whose overlap with compute depends on the process's hardware-queue count:
 * DESIGN.md section 6).  Either pointer may be the host one; no synchronisation.                                               */
int orbhip_copy_pinned_async(void* dst, const void* src, size_t bytes, void* stream);

/* ---------------------------------------------------------------- extractor --
 * Replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-111,
 * src/ORBextractor.cc:410-470 ctor, :1043-1105 operator()).                     */
typedef struct orbx_ctx orbx_ctx;

/* cv::KeyPoint's seven fields, 28 bytes (pt.x, pt.y, size, angle, response, octave, class_id) */
typedef struct orbx_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbx_keypoint;

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (src/ORBextractor.cc:410-470); `device` = HIP device ordinal.  Capacity: per-level quotas up to about 3200 keypoints keep
 * the octree's node arrays in LDS; larger ones (nfeatures beyond ~15000) run the same kernel on a global scratch row per
 * (frame, level), up to 32752 keypoints in one level (16-bit node indices; ORBHIP_EINVAL from the first extract call beyond
 * that - an error, never silent).  The number of FAST corners per level is not limited (candidate arrays are sized for the
 * worst case of the image geometry).                                                                                      */
int orbx_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast, int device,
                orbx_ctx** out);
int orbx_destroy(orbx_ctx* ctx);

/* GetLevels / GetScaleFactor(s) / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:63-83) plus the per-level quotas
 * mnFeaturesPerLevel (:435-446).  Any pointer may be NULL.                        */
int orbx_get_levels(const orbx_ctx* ctx);
int orbx_get_tables(const orbx_ctx* ctx, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                    int32_t* features_per_level);
/* upper bound on keypoints per frame (nfeatures + 3 per level): size outputs with this */
int orbx_max_keypoints(const orbx_ctx* ctx);

/* operator()(image, mask, keypoints, descriptors) for ONE host image (src/ORBextractor.cc:1043-1105).
 * img: CV_8UC1 rows of `stride` bytes.  Empty image (w<=0 or h<=0 or img==NULL) -> returns 0 with *n = 0 and
 * kps / desc32 untouched (":1046": the reference returns without touching its outputs; the C++ shim keeps the caller's
 * vector as it is in that case).  kps[cap], desc32[cap*32].                                */
int orbx_extract(orbx_ctx* ctx, const uint8_t* img, int w, int h, int stride, orbx_keypoint* kps,
                 uint8_t* desc32, int cap, int* n);

/* Batched, device-resident form: nframes images of the same size, frame f at
 * d_imgs + f*frame_stride_bytes.  Outputs (device): d_kps[nframes*cap], d_desc[nframes*cap*32],
 * d_counts[nframes] (keypoints per frame; -1 = that frame hit ORBHIP_EOVERFLOW).
 * Only enqueues on `stream`.                                                      */
int orbx_extract_batch_device(orbx_ctx* ctx, const uint8_t* d_imgs, int w, int h, int stride,
                              size_t frame_stride_bytes, int nframes, orbx_keypoint* d_kps, uint8_t* d_desc,
                              int cap, int32_t* d_counts, void* stream);

/* mvImagePyramid (include/ORBextractor.h:85) of the last extract call: copies level `level` of frame
 * `frame` to host (dense, w*h bytes).  blurred=1 returns the 7x7 Gaussian-blurred level that BRIEF
 * sampled (src/ORBextractor.cc:1085-1086).  out may be NULL to query the size.   */
int orbx_get_level_image(orbx_ctx* ctx, int frame, int level, int blurred, uint8_t* out, int* w, int* h);
/* introspection of the last call, for stage-by-stage parity tests: per-level FAST candidates in
 * candidate order as int32 triples (x, y, score) in detection-window coordinates
 * (src/ORBextractor.cc:789-829) and per-level selected keypoints (after DistributeOctTree, :834) as
 * int32 triples in the same coordinates.  out may be NULL; *n returns the count. */
int orbx_get_level_candidates(orbx_ctx* ctx, int frame, int level, int32_t* out, int cap, int* n);
int orbx_get_level_selected(orbx_ctx* ctx, int frame, int level, int32_t* out, int cap, int* n);

/* Measurement hook (no reference counterpart): when enabled, every batch call records HIP events on
 * its stream around its five stages {pyramid, FAST cells, octree, blur, orientation+BRIEF};
 * orbx_get_stage_ms synchronises on the last event, returns the per-stage sums (ms) over the calls
 * made since enabling and the number of calls, then resets.                           */
/* Which OpenCV the pixel arithmetic restates.  The reference's front-end arithmetic lives in OpenCV (cv::resize, cv::GaussianBlur,
 * cv::FAST), whose fixed-point rounding differs between versions; the library's default is what OpenCV 2.4.x / 3.0 - 3.4.1 compute
 * (the reference's README names 2.4.11 and 3.2).  An integrator whose OpenCV is newer selects its GaussianBlur here - tools/pin
 * (pin_extractor) tells which one the installed OpenCV implements:
 *   ORBX_CV_BLUR_8BIT    7x7 sigma-2 taps cvRound(g * 256) = {18,34,49,55,49,34,18} (sum 257), two passes, (sum + 2^15) >> 16
 *   ORBX_CV_BLUR_FIXED16 the "bit-exact" ufixedpoint16 path (OpenCV >= 3.4.2 / 4.x): 8.8 fixed-point taps, error-diffused so that they
 *                        sum to 256: {18,34,48,56,48,34,18}; same two passes and final rounding.  Restated from the published
 *                        algorithm, NOT verified against a build of that OpenCV here: run tools/pin before relying on it.
 * Applies to the calls made after it; the oracle has the same switch (orc_set_blur_variant).                                 */
#define ORBX_CV_BLUR_8BIT 0
#define ORBX_CV_BLUR_FIXED16 1
int orbx_set_opencv_variant(orbx_ctx* ctx, int blur_variant);

#define ORBX_NSTAGES 5
int orbx_set_profiling(orbx_ctx* ctx, int enable);
int orbx_get_stage_ms(orbx_ctx* ctx, float* ms /*[ORBX_NSTAGES]*/, int* ncalls);

/* ------------------------------------------------------------------ matcher --
 * Replaces the distance core of ORB_SLAM2::ORBmatcher (src/ORBmatcher.cc).        */

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1422-1437); host pointers, 32 bytes each. */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* best / second-best Hamming distance of every query against its candidate list, first minimum
 * wins (the inner loop of every Search* method, e.g. src/ORBmatcher.cc:192-208).
 * cand_offsets (nq+1) / cand_idx = CSR candidate lists; both NULL = brute force over all nt targets.
 * Outputs per query: best_idx (-1 = no candidate), best_d, second_d (256 = none). Device pointers. */
int orbm_hamming_best2_device(const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                              const uint32_t* d_cand_offsets, const uint32_t* d_cand_idx, int32_t* d_best_idx,
                              int32_t* d_best_d, int32_t* d_second_d, void* stream);
/* same with host pointers (synchronous) */
int orbm_hamming_best2(const uint8_t* q, int nq, const uint8_t* t, int nt, const uint32_t* cand_offsets,
                       const uint32_t* cand_idx, int32_t* best_idx, int32_t* best_d, int32_t* second_d);

/* Brute-force frame-to-frame matching, batched: pair p matches the keypoints of frame a[p] against
 * frame b[p] of one extract batch: best/second-best over ALL keypoints of b, accept iff
 * best <= th && best < ratio*second (src/ORBmatcher.cc:210-212), then the rotation-consistency
 * histogram filter (ComputeThreeMaxima, :1386-1418; idiom :217-252) when check_ori != 0.
 * d_kps/d_desc/d_counts are orbx_extract_batch_device's outputs (cap = per-frame capacity).
 * d_match12[npairs*cap]: index into frame b or -1.  d_nmatch[npairs].              */
int orbm_match_frames_batch_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                                   int cap, const int32_t* d_pair_a, const int32_t* d_pair_b, int npairs,
                                   float ratio, int th, int check_ori, int32_t* d_match12, int32_t* d_nmatch,
                                   void* stream);

/* ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:363-468) on flattened frames (host pointers).
 * kps = n x 4 floats (x, y, octave, angle) of the undistorted keypoints; bounds2 = {min_x,max_x,min_y,max_y}
 * of frame 2 (Frame::ComputeImageBounds); prev_matched (n1 x 2) is updated in place; matches12[n1].
 * The frame grid, the window lists and every candidate distance are computed on the GPU; the order-dependent pass
 * (":408", ":421-427") runs on the host in frame-1 order.  Returns the match count in *nmatches. */
int orbm_search_for_initialization(const float* kps1, const uint8_t* desc1, int n1, const float* kps2,
                                   const uint8_t* desc2, int n2, const float* bounds2, float* prev_matched,
                                   int window, float nnratio, int check_ori, int32_t* matches12, int* nmatches);

/* Projection-guided searches on flattened data (host pointers).  One engine covers
 *   SearchByProjection(Frame&, vector<MapPoint*>&, th)            src/ORBmatcher.cc:42-119   (mode_best2 = 1, th = TH_HIGH)
 *   SearchByProjection(Frame& cur, const Frame& last, th)         :1161-1271  (best only, TH_HIGH, rotation check)
 *   SearchByProjection(Frame&, KeyFrame*, set&, th, ORBdist)      :1273-1384  (best only, th = ORBdist, rotation check)
 *   SearchByProjection(KeyFrame*, Scw, points, matched, th)       :258-361    (q_pred_level post-filter, TH_LOW)
 *   the candidate selection of Fuse (:724-954; chi2_gate = 5.99) and of SearchBySim3 (:956-1159, called twice).
 * The caller keeps the reference's own geometry (projection, frustum / distance / viewing-angle gates,
 * PredictScale) and passes per query: projected position, window radius, the GetFeaturesInArea level
 * range (-1,-1 = none), an optional predicted level for the [pred-1, pred] post-filter, the descriptor,
 * q_valid (0 = query skipped).  Targets: kps4 = n x {x, y, octave, angle} of the undistorted keypoints,
 * bounds = {min_x, max_x, min_y, max_y}.  Candidates come from the 64x48 grid (Frame::GetFeaturesInArea,
 * src/Frame.cc:243-307), distances from the GPU, and the order-dependent greedy pass runs in query order:
 * `taken` (nullable, n bytes, in/out) marks targets that already hold a map point (skipped; set on
 * assignment, cleared again if the rotation histogram rejects the match).  Outputs: q_match[nq] = target
 * index or -1, q_best_dist[nq] (nullable), *nmatches.                                        */
/* q_valid[q] (nullable = all 1): 0 = skip the query; bit 0 = search; bit 1 (value 3) = search, but a match does NOT close the
 * target for later queries - the reference closes a feature only while its map point has Observations() > 0
 * (src/ORBmatcher.cc:83-84, :1220-1221).  q_match[q] = target index, -1 = none, or -2 - target for a match the rotation
 * histogram removed (the reference had assigned that slot and resets it to nullptr, :1260-1264; *nmatches does not count it). */
int orbm_search_by_projection(const float* kps4, const uint8_t* desc, int n, const float* bounds, const float* q_uv,
                              const float* q_radius, const int32_t* q_min_level, const int32_t* q_max_level,
                              const int32_t* q_pred_level, const uint8_t* q_desc, const uint8_t* q_valid,
                              const float* q_angle, int nq, const float* inv_level_sigma2, float chi2_gate,
                              uint8_t* taken, int mode_best2, float ratio, int th, int check_ori, int32_t* q_match,
                              int32_t* q_best_dist, int* nmatches);

/* ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:956-1159) on flattened data (host pointers), whole entry point from the two
 * window searches on.  The caller keeps the reference's geometry (transform with sR21 / sR12, depth / image / distance gates,
 * PredictScale) and passes, per feature of keyframe 1 that holds a usable, not yet matched map point (q12_valid), its
 * projection into keyframe 2, the radius th * scale_factors_[predicted level] and the predicted level - and the same for
 * keyframe 2 into keyframe 1 (q21_*).  desc1 / desc2 = the keyframes' own descriptors (the search targets); q12_desc[n1][32] /
 * q21_desc[n2][32] = pMP->GetDescriptor() of the feature's map point (":1036", ":1112"; NULL = the keyframe's own row).  Each
 * direction takes the best candidate of KeyFrame::GetFeaturesInArea with level in [pred - 1, pred] and distance <= TH_HIGH; a
 * pair is kept iff the two directions agree (:1145-1157).  match12[n1] = index in keyframe 2 or -1; *nfound = the return value.
 * bounds1[4] / bounds2[4] = {min_x, max_x, min_y, max_y} of keyframe 1 / 2: each window search runs on the TARGET keyframe's own
 * grid (pKF2->GetFeaturesInArea :1022, pKF1->GetFeaturesInArea :1102). */
int orbm_search_by_sim3(const float* kps1, const uint8_t* desc1, int n1, const float* kps2, const uint8_t* desc2, int n2,
                        const float* bounds1, const float* bounds2, const float* q12_uv, const float* q12_radius, const int32_t* q12_pred,
                        const uint8_t* q12_valid, const uint8_t* q12_desc, const float* q21_uv, const float* q21_radius,
                        const int32_t* q21_pred, const uint8_t* q21_valid, const uint8_t* q21_desc, int32_t* match12, int* nfound);

/* SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBmatcher.cc:151-256; strict = 0) and SearchByBoW(KeyFrame*,
 * KeyFrame*, ...) (:470-580; strict = 1: best < th) on flattened data (host pointers).  The DBoW2 feature
 * vectors are passed as ascending node ids with CSR keypoint-index lists; valid1/valid2 (nullable) mark
 * keypoints that hold a usable map point.  match12[n1] = index in set 2 or -1.               */
int orbm_search_by_bow(const uint8_t* desc1, int n1, const uint8_t* valid1, const float* angle1, const uint8_t* desc2,
                       int n2, const uint8_t* valid2, const float* angle2, const uint32_t* fv1_node,
                       const uint32_t* fv1_off, const uint32_t* fv1_idx, int fv1_n, const uint32_t* fv2_node,
                       const uint32_t* fv2_off, const uint32_t* fv2_idx, int fv2_n, float ratio, int th, int strict,
                       int check_ori, int32_t* match12, int* nmatches);

/* ---- LocalMapping::CreateNewMapPoints, per-match body (src/LocalMapping.cc:267-378, monocular): ray-parallax
 * test, linear triangulation (null vector of the 4x4 system; the reference uses Eigen::JacobiSVD<Matrix4d>), positive depth in
 * both keyframes, chi-square reprojection gates (5.991 * level_sigma2), scale consistency.  Tcw = [Rcw | tcw] row-major 3x4 of
 * the current (1) and the neighbour (2) keyframe; kp1 / kp2 = n x {x, y, octave} floats of the matched undistorted keypoints
 * (matched_indices_ already applied); ratio_factor = 1.5f * scale_factor_.  ok[i] = 1 and x3D[i] valid for accepted matches. */
int orbm_triangulate_matches(const double* Tcw1, const double* Tcw2, const float* K1, const float* K2, const float* kp1,
                             const float* kp2, int n, const float* level_sigma2, const float* scale_factors, int n_levels,
                             float ratio_factor, double* x3D, uint8_t* ok);

/* ---- Frame::ComputeBoW: DBoW2 TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup)
 * (lib/DBoW2/DBoW2/TemplatedVocabulary.h:1124-1260), TF_IDF weighting + L1 norm as ORBVocabulary uses.  The tree is given
 * flattened, node 0 = root: node_desc[n_nodes][32], children of node i = children[child_off[i] .. child_off[i+1]) in their
 * stored order (a leaf has none), word_id / weight of the leaves (word id of an inner node is ignored), L = depth.        */
typedef struct orbv_ctx orbv_ctx;
int orbv_create(const uint8_t* node_desc, const uint32_t* child_off /*[n_nodes+1]*/, const uint32_t* children,
                const int32_t* word_id, const double* weight, int n_nodes, int L, int device, orbv_ctx** out);
int orbv_destroy(orbv_ctx* ctx);
/* ORBVocabulary::loadFromTextFile (lib/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1423) - ORBvoc.txt straight into the device-resident
 * flattened tree: header "k L scoring weighting", then one node per line "parent is_leaf d0 .. d31 weight" (node ids in file
 * order from 1, children in file order, word ids in file order).  orbv_parse_text is the host half alone (arrays allocated with
 * malloc, release each with orbv_free_parsed); blank lines are skipped (the reference's eof loop turns the trailing one into a
 * spurious child of the root with an uninitialised descriptor - not reproduced).                                              */
int orbv_load_text(const char* path, int device, orbv_ctx** out);
int orbv_parse_text(const char* path, int32_t* k, int32_t* L, int32_t* scoring, int32_t* weighting, int32_t* n_nodes, int32_t* n_children,
                    uint8_t** node_desc, uint32_t** child_off, uint32_t** children, int32_t** word_id, double** weight);
void orbv_free_parsed(void* p);
/* desc[n][32] -> BowVector as ascending (bow_word[k], bow_value[k]), k < *n_words <= n, and FeatureVector as CSR:
 * node ids fv_node[m] ascending, features fv_idx[fv_off[m] .. fv_off[m+1]) ascending, m < *n_fv_nodes <= n (fv_off has n+1
 * entries) - the layout orbm_search_by_bow / orbm_search_for_triangulation take.  src/Frame.cc:322-327 uses levelsup = 4.
 * The node of a feature whose leaf lies above level L - levelsup is 0 (the reference leaves it uninitialised there).     */
int orbv_transform(orbv_ctx* ctx, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word, double* bow_value,
                   int* n_words, uint32_t* fv_node, uint32_t* fv_off, uint32_t* fv_idx, int* n_fv_nodes);
/* the tree descent only, device-resident and batchable over frames: per feature its word id, idf weight and node id.
 * Enqueue only.                                                                                                          */
int orbv_descend_device(orbv_ctx* ctx, const uint8_t* d_desc, int n, int levelsup, int32_t* d_word, double* d_weight,
                        uint32_t* d_node, void* stream);
/* L1Scoring::score (lib/DBoW2/DBoW2/ScoringObject.cpp:23-68) between two BowVectors in the layout above (host arithmetic). */
double orbv_score_l1(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2);

/* ---- KeyFrameDatabase (src/KeyFrameDatabase.cc, all of it; DESIGN.md section 2 "KeyFrameDatabase"): the loop and relocalisation
 * candidates, computed by scanning every stored BowVector against the query on the device.  A keyframe is a `slot` (a non-negative
 * index the caller chooses; the tables grow to the largest one).  BowVectors are ascending word ids below n_words with double values,
 * as orbv_transform returns them.  Lists come back in the reference's order: first touch while the query's words are walked in
 * ascending id and each word's list in `add` order, i.e. by (smallest word shared with the query, `add` sequence number).
 * Scores are float(L1Scoring::score), bit for bit.
 *
 * A database is used by one host thread at a time.  create / clear / size keep host state only and work without a device; every other
 * entry returns ORBHIP_ENODEV without one, after its arguments have been checked (ORBHIP_EINVAL first).  add / erase /
 * set_best_covisibles / clear complete before they return; they must not be called while a _batch_device call is still in flight.
 *
 * Query stamps: the reference stamps keyframes with the query's id and compares against fields that start at 0.  Every query takes a
 * query_id; per kind (loop, relocalisation) an id that is not positive or not greater than the last one used is ORBHIP_EINVAL.  An
 * id counts as used once a call's arguments have passed, whatever happens later in that call.  A batch uses first_query_id ..
 * first_query_id + n_queries - 1.  clear forgets the ids and all per-slot state.                                                  */
typedef struct orbv_db orbv_db;
typedef struct orbv_db_query_info {       /* per query (the batched entries write one per query to device memory) */
  int32_t max_common;                     /* maxCommonWords over the sharing list */
  int32_t n_sharing;                      /* length of keyframes_sharing_words */
  int32_t n_scored;                       /* keyframes above minCommonWords (nscores) */
  int32_t n_kept;                         /* length of score_and_matches (loop: score >= minScore) */
  int32_t n_cand;                         /* candidates returned (or wanted, when status is ORBHIP_ECAP) */
  int32_t status;                         /* 0, or ORBHIP_ECAP: n_cand > cap, no candidate of this query was written */
  float best_acc;                         /* bestAccScore (0 when nothing was kept) */
  int32_t min_common;                     /* int(max_common * 0.8f) */
} orbv_db_query_info;
/* Optional trace of a host query: info and the kept list in order - slot, score, accumulated score, best keyframe of its neighbourhood.
 * Every pointer nullable; ORBHIP_ECAP (nothing written) when n_kept > kept_cap.                                                    */
typedef struct orbv_db_trace {
  orbv_db_query_info* info;
  int32_t* kept_slot; float* kept_score; float* kept_acc; int32_t* kept_best;
  int32_t kept_cap, reserved;
} orbv_db_trace;
int orbv_db_create(int n_words, int device, orbv_db** out);
int orbv_db_destroy(orbv_db* db);
int orbv_db_clear(orbv_db* db);
/* ORBHIP_EINVAL for a slot that is in the database, words that do not ascend, a word id not below n_words.  A slot erased and added
 * again goes to the back of every word's list (it gets a new sequence number); its reloc_query / reloc_score stay, as the fields of the
 * reference's KeyFrame do.  Erasing a slot that is not in the database does nothing.  orbv_db_size returns the number of keyframes in
 * the database.  Erased BowVectors are compacted away once they are more than half of the stored ones.                             */
int orbv_db_add(orbv_db* db, int slot, const uint32_t* words, const double* values, int n);
int orbv_db_erase(orbv_db* db, int slot);
int orbv_db_size(const orbv_db* db);
/* GetBestCovisibilityKeyFrames(10) of a slot, resident: n <= 10 slots in that order.  A neighbour that is not in the database when a
 * query runs contributes nothing.                                                                                                 */
int orbv_db_set_best_covisibles(orbv_db* db, int slot, const int32_t* neigh, int n);
/* reloc_query_ / reloc_score_ of the listed slots (the reference never initialises reloc_score_; here both start at 0). */
int orbv_db_get_state(orbv_db* db, const int32_t* slots, int n, int64_t* reloc_query, float* reloc_score);
/* LoopClosing::DetectLoop's minScore (src/LoopClosing.cc:127-139): the lowest float score of the query against the listed slots (the
 * covisible keyframes that are not bad), starting from 1.0f.  ORBHIP_EINVAL for a slot that is not in the database.              */
int orbv_db_min_score(orbv_db* db, const uint32_t* words, const double* values, int n, const int32_t* slots, int n_slots, float* min_score);
/* DetectLoopCandidates(keyframe, minScore) / DetectRelocalizationCandidates(frame): host pointers, one call, one synchronisation.
 * connected = the slots of keyframe->GetConnectedKeyFrames().  Neighbours come from the resident table.  ORBHIP_ECAP, with nothing
 * written, when the candidates exceed cap.  A query BowVector of more than 4096 words is searched in global memory instead of LDS
 * (slower, same result).                                                                                                         */
int orbv_db_detect_loop_candidates(orbv_db* db, const uint32_t* words, const double* values, int n, const int32_t* connected, int n_connected, float min_score,
                                   int64_t query_id, int32_t* cand, int cap, int32_t* n_cand, const orbv_db_trace* trace);
int orbv_db_detect_relocalization_candidates(orbv_db* db, const uint32_t* words, const double* values, int n, int64_t query_id, int32_t* cand, int cap,
                                             int32_t* n_cand, const orbv_db_trace* trace);
/* The same in two halves, for callers whose covisibility graph lives in host objects: _begin returns the kept list (score_and_matches)
 * in order; the caller supplies GetBestCovisibilityKeyFrames(10) of exactly those keyframes as rows[n_kept][10] / row_n[n_kept] (slots);
 * _finish accumulates over them and returns the candidates.  The same kernels as the one-call forms.  add / erase / clear /
 * set_best_covisibles or another query between the halves cancel the pending query (_finish: ORBHIP_EINVAL).                       */
int orbv_db_detect_loop_candidates_begin(orbv_db* db, const uint32_t* words, const double* values, int n, const int32_t* connected, int n_connected,
                                         float min_score, int64_t query_id, int32_t* kept, int kept_cap, int32_t* n_kept);
int orbv_db_detect_relocalization_candidates_begin(orbv_db* db, const uint32_t* words, const double* values, int n, int64_t query_id, int32_t* kept,
                                                   int kept_cap, int32_t* n_kept);
int orbv_db_detect_candidates_finish(orbv_db* db, const int32_t* rows, const int32_t* row_n, int32_t* cand, int cap, int32_t* n_cand, const orbv_db_trace* trace);
/* Between _begin and _finish: the fields the reference writes to the keyframes it touches, per slot 0 .. S-1 (S = highest slot ever used + 1;
 * ORBHIP_ECAP when cap < S): n_common[s] = n_loop_words_ / n_reloc_words_ (0: the query did not stamp the slot - it shares no word, is not in
 * the database, or is connected to the loop query), score[s] = loop_score_ / reloc_score_ where n_common[s] > info->min_common (not meaningful
 * elsewhere).  *info: the counters known so far.                                                                                    */
int orbv_db_pending_fields(orbv_db* db, orbv_db_query_info* info, int32_t* n_common, float* score, int cap);
/* n_queries queries with DEVICE pointers, enqueued on `stream` (no allocation, no host synchronisation): query q's BowVector is
 * entries q_off[q] .. q_off[q+1] of q_words / q_values, its connected slots conn_off[q] .. conn_off[q+1] of conn, its minScore
 * min_score[q]; out info[q] and cand[q][cap] (n_cand of them).  The scan and the scores are batched over the queries; ordering,
 * accumulation and the relocalisation state run per query in stream order, so the result and the state left behind are those of
 * n_queries single calls in the same order, bit for bit.  The BowVectors are not read on the host: they must ascend.
 * `workspace`: device memory of orbv_db_detect_workspace() bytes (which grows with the database: ask again after add), 256-byte
 * aligned, not shared with concurrent calls.                                                                                      */
int orbv_db_detect_loop_candidates_batch_device(orbv_db* db, int n_queries, const int32_t* d_q_off, const uint32_t* d_q_words, const double* d_q_values,
                                                const int32_t* d_conn_off, const int32_t* d_conn, const float* d_min_score, int64_t first_query_id,
                                                orbv_db_query_info* d_info, int32_t* d_cand, int cap, void* d_workspace, size_t workspace_bytes, void* stream);
int orbv_db_detect_relocalization_candidates_batch_device(orbv_db* db, int n_queries, const int32_t* d_q_off, const uint32_t* d_q_words,
                                                          const double* d_q_values, int64_t first_query_id, orbv_db_query_info* d_info, int32_t* d_cand,
                                                          int cap, void* d_workspace, size_t workspace_bytes, void* stream);
int orbv_db_detect_workspace(const orbv_db* db, int n_queries, size_t* bytes);

/* ---- the steps either side of extract -> match: undistortion, the 64 x 48 frame grid, window candidates,
 * frustum test.  kps4 = n x {x, y, octave, angle} floats of the UNDISTORTED keypoints; bounds = {min_x, max_x, min_y, max_y}
 * (Frame::ComputeImageBounds, src/Frame.cc:357-385).  Host pointers; the arithmetic runs on the device.                  */

/* Frame::UndistortKeyPoints (src/Frame.cc:329-355): cv::undistortPoints(mat, mat, K, dist, Mat(), K) on n points,
 * dist5 = {k1, k2, p1, p2, k3}; k1 == 0 copies the input, as the reference does.                                        */
int orbm_undistort_keypoints(const float* xy, int n, const float* K4 /*fx,fy,cx,cy*/, const float* dist5, float* xy_out);

/* Frame::AssignFeaturesToGrid (src/Frame.cc:158-173, PosInGrid :309-320): cell c = x * 48 + y holds keypoint indices
 * cell_idx[cell_offsets[c] .. cell_offsets[c+1]) in push_back order; keypoints outside the grid are skipped.            */
int orbm_assign_features_to_grid(const float* kps4, int n, const float* bounds, uint32_t* cell_offsets /*[64*48+1]*/,
                                 uint32_t* cell_idx /*[n]*/, int* n_assigned);

/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:243-307) for nq queries -> CSR lists in the
 * reference's order (cells ix-major then iy, entries in keypoint-index order).  q_min_level / q_max_level NULL = -1 / -1,
 * which is also KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:575-622).  cand_idx may be NULL to size: *total is always set;
 * ORBHIP_ECAP if cap < *total with cand_idx given.                                                                       */
int orbm_features_in_area(const float* kps4, int n, const float* bounds, const float* q_xy, const float* q_radius,
                          const int32_t* q_min_level, const int32_t* q_max_level, int nq, uint32_t* cand_offsets /*[nq+1]*/,
                          uint32_t* cand_idx, int cap, int* total);

/* Frame::isInFrustum (src/Frame.cc:191-241) + MapPoint::PredictScale (src/MapPoint.cc:406-420) for n map points:
 * Rcw (row-major 3x3), tcw of the frame; P = world position, Pn = mean viewing direction, min_dist / max_dist = the map
 * point's raw min_distance_ / max_distance_ (the 0.8 / 1.2 invariance factors are applied here).  Outputs per point:
 * in_view (is_track_in_view_), uv (track_proj_x_, track_proj_y_), level (track_scale_level_), view_cos (track_view_cos_);
 * uv / level / view_cos are written for every point, meaningful where in_view is set.                                    */
int orbm_is_in_frustum(const double* Rcw, const double* tcw, const float* K4, const float* bounds, const double* P,
                       const double* Pn, const float* min_dist, const float* max_dist, int n, float viewing_cos_limit,
                       float log_scale_factor, int n_levels, uint8_t* in_view, float* uv, int32_t* level, float* view_cos);
/* The same gates fed from MapPoint's PUBLIC accessors: min / max = GetMinDistanceInvariance() / GetMaxDistanceInvariance()
 * (min_distance_ / max_distance_ are protected, include/MapPoint.h:125-151), and dist = |P - Ow| as float comes back so that
 * the caller runs MapPoint::PredictScale(dist, frame) itself for the points in view (src/Frame.cc:231).                   */
int orbm_is_in_frustum_gates(const double* Rcw, const double* tcw, const float* K4, const float* bounds, const double* P,
                             const double* Pn, const float* min_dist_invariance, const float* max_dist_invariance, int n,
                             float viewing_cos_limit, uint8_t* in_view, float* uv, float* view_cos, float* dist);

/* SearchForTriangulation (src/ORBmatcher.cc:582-722, mono) on flattened data (host pointers): BoW-node brute force
 * between keypoints WITHOUT a map point (unmapped1/2 flags), dist <= TH_LOW with later ties replacing earlier ones
 * (":654"), rejection near the epipole (ex, ey; ":658-664") and the epipolar-line gate CheckDistEpipolarLine
 * (":128-149") with F12 row-major (3x3 doubles), scale_factors / level_sigma2 of keyframe 2.  Queries are
 * independent (vbMatched2 is never set in this fork).  match12[n1] = index in keyframe 2 or -1.          */
int orbm_search_for_triangulation(const float* kps1, const uint8_t* desc1, const uint8_t* unmapped1, int n1,
                                  const float* kps2, const uint8_t* desc2, const uint8_t* unmapped2, int n2,
                                  const uint32_t* fv1_node, const uint32_t* fv1_off, const uint32_t* fv1_idx, int fv1_n,
                                  const uint32_t* fv2_node, const uint32_t* fv2_off, const uint32_t* fv2_idx, int fv2_n,
                                  const double* F12, float ex, float ey, const float* scale_factors,
                                  const float* level_sigma2, int check_ori, int32_t* match12, int* nmatches);

/* ---- Tracking::Relocalization, first stage (src/Tracking.cc:979-1029; round 5): current_frame_.ComputeBoW() and
 * matcher.SearchByBoW(keyframe, current_frame_, map_point_matches_vector[i]) - ORBmatcher(0.75, true) - for EVERY candidate keyframe of
 * KeyFrameDatabase::DetectRelocalizationCandidates in ONE call (the candidates are independent; the vocabulary descent of the frame
 * runs once).  img != NULL: the frame is extracted first and stays on the device (as orbt_track_reference_keyframe); NULL: the
 * frame an earlier orbt_* call of this thread left there.  Per candidate i: slot_owner[i][f] = the keyframe feature whose map
 * point vpMapPointMatches[f] holds (-1: none) after the rotation check, nmatches[i] = the return value (the caller discards the
 * candidate below 15, :1019).  What follows - PnPsolver::iterate per candidate, then PoseOptimization /
 * SearchByProjection(F, KF, found, th, ORBdist) rounds (:1040-1120) - is made of two further calls: orbt_pnp_iterate_batch_device runs
 * one PnPsolver::iterate of every candidate, and orbt_relocalization_refine (below) runs everything behind a PnP pose for every
 * candidate that has one, on the frame this call left on the device. */
typedef struct orbt_reloc_keyframe {
  const uint8_t* desc; const uint8_t* valid; const float* angle; int n;      /* descriptors, 1 = usable map point (not NULL, not isBad()), keypoint angles */
  const uint32_t* fv_node; const uint32_t* fv_off; const uint32_t* fv_idx; int fv_n;      /* the keyframe's FeatureVector (orbv_transform's layout) */
} orbt_reloc_keyframe;
int orbt_relocalization_search_by_bow(orbx_ctx* ctx, orbv_ctx* voc, const uint8_t* img, int w, int h, int stride, const float* K4, const float* bounds,
                                      const orbt_reloc_keyframe* candidates, int n_candidates, float nnratio, int check_ori, orbx_keypoint* kps_out,
                                      uint8_t* desc_out, int cap, uint32_t* bow_word, double* bow_value, int* n_words, uint32_t* fv_node, uint32_t* fv_off,
                                      uint32_t* fv_idx, int* n_fv_nodes, int32_t* slot_owner /*[n_candidates][cap]*/, int32_t* nmatches /*[n_candidates]*/,
                                      int* n_keypoints);

/* ---- Tracking::Relocalization behind a PnP pose (src/Tracking.cc:1056-1126), for EVERY candidate of a `while` round in ONE call on
 * the resident frame: PoseOptimization, SearchByProjection(F, KF, found, 10, 100), PoseOptimization, SearchByProjection(F, KF, found,
 * 3, 64), PoseOptimization, with the gates `< 10`, `< 50`, `nadditional + nGood >= 50`, `30 < nGood < 50` and `>= 50` decided on the
 * device: one upload, a fixed sequence of 14 launches whatever the sizes, one download, one synchronisation.  The candidates are
 * independent (:1066-1072 overwrites every slot per candidate), so all of them are refined and *first_match is the lowest index with
 * nGood >= 50 (-1: none): the candidate at which the reference breaks out of its loop.  The caller takes that candidate's outputs.
 *   per candidate  n <= 4096 keyframe features; per feature i: pt[i] = an id (>= 0, any value) of the map point in
 *        GetMapPointMatches()[i], -1 for NULL or isBad() - `found` is a set of these ids, so a point held at two features behaves as
 *        in the reference's std::set<MapPoint*>; Xw[i][3]; desc[i][32] = MapPoint::GetDescriptor(); min_dist / max_dist = the raw
 *        min_distance_ / max_distance_ (the 0.8 / 1.2 factors are applied inside); angle[i] = undistort_keypoints_[i].angle (the
 *        five arrays are read where pt[i] >= 0).  Tcw = the PnP pose, row-major 3x4 (or the first 12 of a 4x4); NULL: the candidate has
 *        no pose in this round and is not refined.  slot_kf[n_kp] = the keyframe feature whose point current_frame_.map_points_[f]
 *        holds after the is_inliers masking of :1066-1072, -1 none; it must name features with pt >= 0.
 *   call  K4, bounds, log_scale_factor as for orbt_track_local_map; n_kp = the resident frame's keypoint count; check_ori = the
 *        matcher's mbCheckOrientation (the reference: 1); narrow_in_loop = 1: the narrow search sits INSIDE the `for (ip < N_)` loop
 *        as in the reference (:1097-1104) - evaluated exactly as the passes in order, each with `found` as it stands at its ip, up
 *        to the first pass that assigns nothing (every later pass is empty then, and nadditional is 0 unless pass N_ - 1 ran);
 *        0: upstream ORB-SLAM2's placement, ONE search behind the loop with every slot's point in `found`.
 *   out  res[c]: stage (ORBT_RR_*), matched, narrow_passes (passes run, <= N_), n_good[k] / n_correspondences[k] of the k-th
 *        PoseOptimization and n_additional[0] / [1] of the wide / narrow search (-1 where one did not run), pose7 = the pose
 *        current_frame_ ends with; slot_kf_out[c][n_kp] / outlier[c][n_kp] = map_points_ (as keyframe features) and is_outliers_ as
 *        the reference leaves them for that candidate, starting from flags that are all false.  Nothing is written beyond
 *        n_candidates x n_kp entries.  Quirks kept: outlier slots are cleared behind the first and the third solve, not behind the
 *        second; `found` of the wide search is the PnP inlier set with the slots cleared since still in it; a point outside `found`
 *        that already sits in a slot is matched a second time.
 * At most ORBT_RR_MAX_CANDIDATES candidates per call.  ORBHIP_EINVAL, before any device work, for NULL arguments, negative counts,
 * pt[i] < -1, a slot_kf entry out of range or naming a feature without a point (the message names the entry and the array), and -
 * with a device - without a resident frame of ctx on the calling thread or with another n_kp than it has; ORBHIP_ECAP for more than 64
 * candidates or 4096 features; ORBHIP_ENODEV without a GPU.  The call needs no caller scratch.                                      */
#define ORBT_RR_MAX_CANDIDATES 64
#define ORBT_RR_NO_POSE 0         /* no pose, or fewer than 3 correspondences: PoseOptimization returned 0 */
#define ORBT_RR_FEW_INLIERS 1     /* nGood < 10 behind the first solve */
#define ORBT_RR_MATCH_FIRST 2     /* nGood >= 50 behind the first solve */
#define ORBT_RR_MATCH_SECOND 3    /* ... behind the second */
#define ORBT_RR_MATCH_THIRD 4     /* ... behind the third */
#define ORBT_RR_FAIL_WIDE 5       /* nadditional + nGood < 50 behind the wide search: no second solve */
#define ORBT_RR_FAIL_SECOND 6     /* nGood <= 30 behind the second solve: no narrow search */
#define ORBT_RR_FAIL_NARROW 7     /* nGood + nadditional < 50 behind the narrow search: no third solve */
#define ORBT_RR_FAIL_THIRD 8      /* nGood < 50 behind the third solve */
typedef struct orbt_reloc_refine_candidate {
  const int32_t* pt; const double* Xw; const uint8_t* desc; const float* min_dist; const float* max_dist; const float* angle; int32_t n, reserved;
  const double* Tcw; const int32_t* slot_kf;
} orbt_reloc_refine_candidate;
typedef struct orbt_reloc_refine_result {
  int32_t stage, matched, narrow_passes, reserved;
  int32_t n_good[3], n_additional[2], n_correspondences[3];
  double pose7[7];
} orbt_reloc_refine_result;
int orbt_relocalization_refine(orbx_ctx* ctx, const float* K4, const float* bounds, float log_scale_factor, const orbt_reloc_refine_candidate* candidates,
                               int n_candidates, int n_kp, int check_ori, int narrow_in_loop, orbt_reloc_refine_result* res /*[n_candidates]*/,
                               int32_t* slot_kf_out /*[n_candidates][n_kp]*/, uint8_t* outlier /*[n_candidates][n_kp]*/, int32_t* first_match);

/* ---- LocalMapping::CreateNewMapPoints, device-resident across the neighbour keyframes (src/LocalMapping.cc:196-396; round 5) ----
 * For every neighbour keyframe IN ORDER: ORBmatcher::SearchForTriangulation(current, neighbour, F12, pairs, false) with the matcher of
 * that call site, ORBmatcher(0.6, false) (:203: no orientation check; src/ORBmatcher.cc:582-722), then the per-match body (:267-378:
 * ray parallax, linear triangulation, depth / chi-square / scale gates) - and what makes the neighbours depend on each other: a
 * triangulated match gives the current keyframe's keypoint a map point (AddMapPoint, :383), so the next neighbour's search skips it
 * (src/ORBmatcher.cc:621-623).  One upload, one kernel per neighbour on the calling thread's stream, one download; the map mutation
 * (:380-393) is the caller's loop over the accepted entries (csrc/compat/orbslam_dropin.h: CreateNewMapPoints).
 *   current keyframe: kps1[n1][4] = {x, y, octave, angle} undistorted keypoints, desc1[n1][32], unmapped1[n1] (1 = GetMapPoint(idx) ==
 *     NULL; NULL = all), its FeatureVector as ascending node ids + CSR lists (orbv_transform's layout), Tcw1 row-major 3x4, K1 = {fx, fy,
 *     cx, cy}.  Neighbours that fail the baseline test (:231-244) are left out by the caller.
 *   scale_factors / level_sigma2 [n_levels]: the extractor's tables (every keyframe copies them from the same ORBextractor);
 *     ratio_factor = 1.5f * current_keyframe_->scale_factor_ (:221).
 *   stop (nullable): a byte the caller may raise while the call runs = CheckNewKeyFrames() (:227): it is looked at ONCE before every
 *     neighbour after the first; the neighbours before it are complete, *n_processed says how many.
 *   out, per neighbour k and keypoint i of the current keyframe: match12[k][i] = SearchForTriangulation's partner or -1,
 *     ok[k][i] = 1 when the triangulation passed every gate, x3D[k][i] = the new point (zeros otherwise).                       */
typedef struct orbl_keyframe {
  const float* kps; const uint8_t* desc; const uint8_t* unmapped; int n;           /* as kps1 / desc1 / unmapped1 */
  const uint32_t* fv_node; const uint32_t* fv_off; const uint32_t* fv_idx; int fv_n;
  double Tcw[12]; float K4[4];
  double F12[9];              /* LocalMapping::ComputeF12(current, this) (:507-523), row-major */
  float ex, ey;               /* the epipole of the current keyframe's centre in this keyframe (src/ORBmatcher.cc:588-595) */
} orbl_keyframe;
int orbl_create_new_map_points(const float* kps1, const uint8_t* desc1, const uint8_t* unmapped1, int n1, const uint32_t* fv1_node,
                               const uint32_t* fv1_off, const uint32_t* fv1_idx, int fv1_n, const double* Tcw1, const float* K1,
                               const orbl_keyframe* neighbours, int n_neighbours, const float* scale_factors, const float* level_sigma2,
                               int n_levels, float ratio_factor, const volatile uint8_t* stop, int32_t* match12, uint8_t* ok, double* x3D,
                               int* n_processed);
/* ---- LocalMapping::SearchInNeighbors (:398-505): the candidate selection of ORBmatcher::Fuse (src/ORBmatcher.cc:724-842) for ALL
 * target keyframes of one loop in ONE call.  The caller keeps the reference's own projection (Rcw p + tcw, IsInImage, the distance
 * and viewing-angle gates, PredictScale: :739-778) and passes, per (keyframe t, map point m), q_uv[t][m] = (u, v), q_radius[t][m] =
 * th * scale_factors_[level], q_level[t][m] = nPredictedLevel or -1 when a gate failed; mp_desc[m] = pMP->GetDescriptor().  The call
 * does KeyFrame::GetFeaturesInArea on every keyframe's own 64 x 48 grid (src/KeyFrame.cc:575-622), the level window (:781), the
 * chi-square gate (:789) and the descriptor distances: best_idx[t][m] = the keypoint (-1: none), best_dist[t][m] (256: none); the
 * caller applies `bestDist <= TH_LOW` and the Replace / AddObservation mutation in the reference's order (:806-823).  A map point
 * whose descriptor changes through such a mutation (MapPoint::Replace recomputes it) is re-queried by the caller for the keyframes
 * that follow (csrc/compat/orbslam_dropin.h).                                                                                    */
typedef struct orbl_fuse_keyframe {
  const float* kps; const uint8_t* desc; int n;      /* undistorted keypoints {x, y, octave, angle}, descriptors */
  float bounds[4];                                   /* {min_x_, max_x_, min_y_, max_y_} */
} orbl_fuse_keyframe;
int orbl_fuse_batch(const orbl_fuse_keyframe* keyframes, int n_keyframes, const float* q_uv, const float* q_radius, const int32_t* q_level,
                    int n_map_points, const uint8_t* mp_desc, const float* inv_level_sigma2, int n_levels, int32_t* best_idx,
                    int32_t* best_dist);
/* ---- LoopClosing::SearchAndFuse (src/LoopClosing.cc:599-630): the candidate selection of ORBmatcher::Fuse(KeyFrame*, Scw, points, th,
 * replace) (src/ORBmatcher.cc:844-954) for ALL corrected keyframes of a loop closure in ONE call.  As orbl_fuse_batch, without the
 * chi-square gate (the Sim(3) form has none): the caller projects with the CORRECTED Sim(3) of every keyframe (Rcw = sRcw / s,
 * tcw = t / s, :854-859) and keeps the gates :873-906; best_idx / best_dist as above; `bestDist <= TH_LOW`, vpReplacePoint /
 * AddObservation and the Replace loop under the map mutex stay with the caller, keyframe after keyframe (csrc/compat/orbslam_dropin.h:
 * ORBmatcher::SearchAndFuse re-queries a point whose descriptor a Replace recomputed and re-reads GetMapPoints() per keyframe).   */
int orbl_fuse_batch_sim3(const orbl_fuse_keyframe* keyframes, int n_keyframes, const float* q_uv, const float* q_radius, const int32_t* q_level,
                         int n_points, const uint8_t* mp_desc, int n_levels, int32_t* best_idx, int32_t* best_dist);

/* ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:256-315) and MapPoint::UpdateNormalAndDepth (:335-378) for a BATCH of
 * npts map points in ONE call: the per-point loops of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:141-152), the tail of
 * CreateNewMapPoints (:386-388), the tail of SearchInNeighbors (:476-485) and the LocalBA write-back (src/CeresOptimizer.cc:590-598).
 * Points are independent; a batch computes what the reference's loop of single calls computes.
 *   what: ORBL_MP_DESC, ORBL_MP_NORMAL_DEPTH or both.
 *   per point p: its observations are obs_off[p] .. obs_off[p+1] (CSR, obs_off[0] = 0, obs_off[npts] = nobs) in the caller's
 *     std::map<KeyFrame*, size_t> iteration order; X[p][3] = world position; ref_kf[p] = index of GetReferenceKeyFrame() in kf_center;
 *     ref_level[p] = the octave of that keyframe's keypoint observations[reference_keyframe] (:369-371; when the reference keyframe is
 *     not in the list, std::map::operator[] on the method's local copy yields index 0: keypoint 0's octave); pt_good[p] (nullable =
 *     all 1) = !isBad().
 *   per observation e: obs_kf[e] = index of the keyframe in kf_center[nkf][3] (GetCameraCenter()), obs_desc[e][32] = that keyframe's
 *     descriptor row (gathered by the caller, :272-279), obs_kf_good[e] (nullable = all 1) = !keyframe->isBad().
 *   scale_factors[n_levels]: the reference keyframe's table (:372-373; every keyframe copies it from the same extractor).
 * Descriptor (:256-315): the observations of good keyframes only, N of them; the row of the N x N Hamming matrix with the least
 *   median (sorted_row[(N - 1) / 2], the diagonal zero included), first row on ties.  best_obs[p] = its position in the point's list
 *   (0-based from obs_off[p]) and desc_out[p][32] = its bytes; best_obs[p] = -1 and desc_out[p] untouched when N = 0, the point is
 *   bad or its list is empty.
 * Normal and depth (:335-378): ALL observations (bad keyframes included): normal[p] = sum (X - O_i) / |X - O_i| / n in double, list
 *   order; dist = (float)|X - O_ref|, min_max[p] = {max / scale_factors[n_levels - 1], max = dist * scale_factors[ref_level]} in
 *   float; nd_written[p] = 1.  Bad points and empty lists: nd_written[p] = 0, normal[p] / min_max[p] untouched.
 * Outputs of a part `what` does not select are not touched and may be NULL, as may the inputs only that part reads (ref_kf,
 * ref_level, X, obs_kf, kf_center, scale_factors for the normal; obs_desc, obs_kf_good for the descriptor).
 * Host pointers, synchronous.  ORBHIP_EINVAL before any device work for negative counts, offsets that do not run monotonically from
 * 0 to nobs, keyframe indices outside [0, nkf) and levels outside [0, n_levels).                                                   */
#define ORBL_MP_DESC 1
#define ORBL_MP_NORMAL_DEPTH 2
int orbl_update_map_points(int npts, const int32_t* obs_off, const double* X, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* pt_good,
                           int nobs, const int32_t* obs_kf, const uint8_t* obs_desc, const uint8_t* obs_kf_good, int nkf, const double* kf_center,
                           const float* scale_factors, int n_levels, int what, int32_t* best_obs, uint8_t* desc_out, double* normal, float* min_max,
                           uint8_t* nd_written);
/* The same with DEVICE pointers, enqueued on `stream` (callers that keep keyframe data resident; the orbm_hamming_best2_device
 * pattern).  `workspace`: device memory of at least orbl_update_map_points_workspace(npts) bytes, not shared with concurrent calls.
 * obs_desc must be 16-byte and desc_out 4-byte aligned.  Counts, NULL pointers and alignment are checked on the host; the data is
 * not read there, so a point whose offsets, keyframe indices or level are out of range is left unchanged (best_obs -1,
 * nd_written 0) instead of failing the call.  best_obs and nd_written are written for every point, the other outputs only where
 * the host entry point writes them.                                                                                              */
int orbl_update_map_points_device(int npts, const int32_t* d_obs_off, const double* d_X, const int32_t* d_ref_kf, const int32_t* d_ref_level,
                                  const uint8_t* d_pt_good, int nobs, const int32_t* d_obs_kf, const uint8_t* d_obs_desc, const uint8_t* d_obs_kf_good,
                                  int nkf, const double* d_kf_center, const float* d_scale_factors, int n_levels, int what, int32_t* d_best_obs,
                                  uint8_t* d_desc_out, double* d_normal, float* d_min_max, uint8_t* d_nd_written, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_update_map_points_device needs for npts points (host arithmetic). */
int orbl_update_map_points_workspace(int npts, size_t* bytes);

/* ---- LocalMapping::KeyFrameCulling (src/LocalMapping.cc:576-637, monocular) for the WHOLE candidate list in ONE call, with the exact
 * sequential semantics of the reference's loop: a culled keyframe's SetBadFlag() (src/KeyFrame.cc:460-480) erases its observations,
 * MapPoint::EraseObservation (src/MapPoint.cc:140-162) turns a point with <= 2 observations left bad, and every LATER candidate counts
 * under that state.
 *   candidates, in the order of GetVectorCovisibleKeyFrames(): cand_kf[c] = keyframe index in [0, nkf); cand_flags[c] (nullable = all
 *     0): bit 0 = id_ == 0 (:588, skipped), bit 1 = do_not_erase_ (SetBadFlag only notes do_to_be_erased_: nothing changes).
 *   slots: slot_off[ncand + 1] (CSR, slot_off[0] = 0); for every non-null entry of the candidate's GetMapPointMatches(), in slot order,
 *     slot_pt[s] = point index in [0, npts) and slot_level[s] = undistort_keypoints_[i].octave.
 *   points: obs_off[npts + 1] (CSR) into obs_kf[e] (the observing keyframe) and obs_level[e] (the octave of that keyframe's keypoint);
 *     pt_bad[p] (nullable = all 0) = isBad(): the lists of bad points are ignored; pt_nobs[p] (nullable = the list length) =
 *     Observations().
 *   th_obs (3 at the call site, >= 1), ratio (0.9).
 * Per candidate c, in order, k = cand_kf[c]:
 *   1. bit 0 set: culled = n_redundant = n_map_points = 0, next candidate.
 *   2. every slot (p, l) whose point is not bad NOW: n_map_points++; if nobs[p] > th_obs and at least th_obs LIVE observations of p
 *      have obs_kf != k and obs_level <= l + 1: n_redundant++.
 *   3. culled = (double)n_redundant > ratio * (double)n_map_points (one IEEE double multiply).
 *   4. culled and bit 1 clear: every point of a slot of c that is not bad and still has a live observation by k (once per point, however
 *      often it is listed) loses that observation and nobs[p]--; when nobs[p] <= 2 the point turns bad and ALL its observations die.
 *      A list that names keyframe k more than once: its first such entry is the keyframe's observation.
 * Outputs: culled[ncand], n_redundant[ncand], n_map_points[ncand] as seen at each candidate's turn; nullable final state
 * pt_bad_out[npts], pt_nobs_out[npts], obs_erased[nobs] (1 = the observation died).  Every output element is written.
 * PRECONDITION for equality with the reference: the map is consistent - keyframe k holds point p in slot i iff p's observations
 * contain (k, i).  The caller then applies SetBadFlag() to the keyframes with culled = 1, in list order.
 * Host pointers, synchronous.  ORBHIP_EINVAL before any device work for negative counts, offsets that do not ascend from 0, indices
 * outside [0, nkf) / [0, npts), negative levels, th_obs < 1, a ratio that is not finite; ORBHIP_ENODEV without a GPU.              */
int orbl_keyframe_culling(int ncand, const int32_t* cand_kf, const uint8_t* cand_flags, const int32_t* slot_off, const int32_t* slot_pt, const int32_t* slot_level,
                          int nkf, int npts, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_level, const uint8_t* pt_bad,
                          const int32_t* pt_nobs, int th_obs, double ratio, uint8_t* culled, int32_t* n_redundant, int32_t* n_map_points, uint8_t* pt_bad_out,
                          int32_t* pt_nobs_out, uint8_t* obs_erased);
/* The same with DEVICE pointers, enqueued on `stream` (nslots = slot_off[ncand], nobs = obs_off[npts] given by the caller).  Counts,
 * NULL pointers and 4-byte alignment of the 32-bit arrays are checked on the host; the data is bounds-checked on the device: an entry
 * that is out of range (offsets, keyframe or point index, negative level) is treated as ABSENT - a slot or observation that is not
 * there, a candidate skipped with zeros - and sets a bit in *d_status (nullable; zeroed first; 1 = offsets, 2 = index, 4 = level).
 * `d_workspace`: at least orbl_keyframe_culling_workspace(...) bytes of device memory, 4-byte aligned, not shared with concurrent calls. */
int orbl_keyframe_culling_device(int ncand, const int32_t* d_cand_kf, const uint8_t* d_cand_flags, int nslots, const int32_t* d_slot_off,
                                 const int32_t* d_slot_pt, const int32_t* d_slot_level, int nkf, int npts, int nobs, const int32_t* d_obs_off,
                                 const int32_t* d_obs_kf, const int32_t* d_obs_level, const uint8_t* d_pt_bad, const int32_t* d_pt_nobs, int th_obs, double ratio,
                                 uint8_t* d_culled, int32_t* d_n_redundant, int32_t* d_n_map_points, uint8_t* d_pt_bad_out, int32_t* d_pt_nobs_out,
                                 uint8_t* d_obs_erased, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_keyframe_culling_device needs (host arithmetic): nine 32-bit arrays - four per slot, two per observation,
 * three per point - each rounded up to 256 bytes; ncand does not enter. */
int orbl_keyframe_culling_workspace(int ncand, int nslots, int npts, int nobs, size_t* bytes);

/* ---- KeyFrame::UpdateConnections (src/KeyFrame.cc:314-398) with AddConnection / UpdateBestCovisibles (:158-193) for a WHOLE list of
 * keyframes in ONE call, with the exact sequential semantics of calling it on each in turn, and the new loop links that
 * LoopClosing::CorrectLoop derives while it walks such a list (src/LoopClosing.cc:551-573).  Keyframes are 0..nkf-1, points 0..npts-1.
 *   targets, in call order: tgt_kf[t] in [0, nkf), distinct; tgt_flags[t] (nullable = all 0): bit 0 = is_first_connection_ && id_ != 0.
 *   slots: slot_off[ntgt + 1] (CSR, slot_off[0] = 0) into slot_pt[s] = the target's map_points_ in slot order: a point index or -1 for a
 *     null slot; a point may be listed twice and then counts twice.
 *   points: pt_bad[p] (nullable = all 0) = isBad(); obs_off[npts + 1] (CSR) into obs_kf[e] = the observing keyframes, in any order.
 *   kf_rank[nkf] (nullable = index order): a permutation, the keyframe's position in the caller's pointer order (std::less<KeyFrame*>).
 *     It is the iteration order of keyframe_counter, breaks the ties of both sort(pairs) calls and orders std::set<KeyFrame*>.
 *   tables of EVERY keyframe at entry: conn_off[nkf + 1] (CSR) into conn_kf[e] / conn_w[e] = connected_keyframe_weights_, in any order
 *     inside a row; a row names a keyframe at most once and never itself.
 *   prev_off[ntgt + 1] / prev_kf[] (nullable as a pair): ordered_connected_keyframes_ of every target at entry; read for the links only.
 *   th: 15 in the reference (:353), >= 1.
 * For each target A in order: 1. every slot of A with a point that is not bad adds one to counter[k] for every observer k != A.
 *   2. empty counter: tgt_status = 1, tgt_parent = -1, nothing of A changes.  3. in ascending kf_rank: the maximum moves on a strictly
 *   greater count (the lowest rank among the maxima wins); every k with counter[k] >= th joins `pairs` and AddConnection(k <- A,
 *   counter[k]) runs; empty `pairs` become {kmax} with AddConnection(kmax <- A, nmax).  4. A's map = the WHOLE counter, A's list = `pairs`
 *   by descending (weight, kf_rank); tgt_parent = the front of that list when bit 0 is set, else -1; tgt_status = 0.
 *   AddConnection(B <- A, w): nothing when B's map holds A with weight w; else map[A] = w and B's list = ALL of B's map by descending
 *   (weight, kf_rank) - the reference's re-sort, which brings entries below th into the list.
 *   Links: with P(A) = A's list as it stands when A's turn begins, link(A) = keys of A's map after its turn \ P(A) \ {every target}.
 * Outputs: tgt_status[ntgt], tgt_parent[ntgt]; counts[4] = {n_aff, n_conn, n_ord, n_link}; the keyframes the loop wrote (own update with a
 * non-empty counter, or an AddConnection that changed something) in ascending index as aff_kf[n_aff]; their new maps as oconn_off[n_aff +
 * 1] / oconn_kf / oconn_w, rows in ascending kf_rank (the map's iteration order); their new lists as oord_off[n_aff + 1] / oord_kf /
 * oord_w; link_off[ntgt + 1] / link_kf (nullable; needs prev_*), rows in ascending kf_rank.  oconn_off / oord_off hold cap_aff + 1 entries,
 * the lists cap_aff / cap_conn / cap_ord / cap_link.  Every element inside the counts is written, nothing beyond them.
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for negative counts or
 * capacities, offsets that do not ascend from 0, ids out of range, duplicate targets, a kf_rank that is not a permutation, a conn row
 * naming a keyframe twice or itself, th < 1, NULL where an array is needed, one of the prev pair without the other, a link output
 * without prev; ORBHIP_ENODEV without a GPU; ORBHIP_ECAP, with only counts[] (the wanted sizes) written, when a list does not fit.  */
int orbl_update_connections(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, const int32_t* slot_off, const int32_t* slot_pt, int nkf, int npts,
                            const int32_t* obs_off, const int32_t* obs_kf, const uint8_t* pt_bad, const int32_t* kf_rank, const int32_t* conn_off,
                            const int32_t* conn_kf, const int32_t* conn_w, const int32_t* prev_off, const int32_t* prev_kf, int th, int cap_aff, int cap_conn,
                            int cap_ord, int cap_link, int32_t* tgt_status, int32_t* tgt_parent, int32_t* aff_kf, int32_t* oconn_off, int32_t* oconn_kf,
                            int32_t* oconn_w, int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w, int32_t* link_off, int32_t* link_kf, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nslots = slot_off[ntgt], nobs = obs_off[npts], nconn =
 * conn_off[nkf], nprev = prev_off[ntgt] given by the caller).  d_counts[4] always holds the WANTED counts.  *d_status (nullable; zeroed
 * first): 1 = offsets, 2 = an index out of range, a kf_rank that is not a permutation or a duplicate target, 4 / 8 / 16 / 32 = cap_aff /
 * cap_conn / cap_ord / cap_link exceeded (the elements below the capacity are still written, none beyond it).  An out-of-range entry is
 * treated as ABSENT (of a keyframe listed twice the last instance counts).  PRECONDITION, not checked here: no conn row names a keyframe
 * twice.  Counts, NULL pointers and 4-byte alignment are checked on the host.  `d_workspace`: at least
 * orbl_update_connections_workspace(...) bytes of device memory, 8-byte aligned, not shared with concurrent calls; it is cleared by every
 * call, so calls may reuse it.                                                                                                        */
int orbl_update_connections_device(int ntgt, const int32_t* d_tgt_kf, const uint8_t* d_tgt_flags, int nslots, const int32_t* d_slot_off,
                                   const int32_t* d_slot_pt, int nkf, int npts, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                   const uint8_t* d_pt_bad, const int32_t* d_kf_rank, int nconn, const int32_t* d_conn_off, const int32_t* d_conn_kf,
                                   const int32_t* d_conn_w, int nprev, const int32_t* d_prev_off, const int32_t* d_prev_kf, int th, int cap_aff, int cap_conn,
                                   int cap_ord, int cap_link, int32_t* d_tgt_status, int32_t* d_tgt_parent, int32_t* d_aff_kf, int32_t* d_oconn_off,
                                   int32_t* d_oconn_kf, int32_t* d_oconn_w, int32_t* d_oord_off, int32_t* d_oord_kf, int32_t* d_oord_w, int32_t* d_link_off,
                                   int32_t* d_link_kf, int32_t* d_counts, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_update_connections_device needs (host arithmetic).  With cells = ntgt * nkf: the votes and the position of
 * every target in every input row (4 bytes per cell each), the link marks (1) and candidates (4), the gathered entries of the final maps
 * (12 bytes for each of nconn + 2 * cells), seven 32-bit words per keyframe and six per target, two per keyframe for the checks - each
 * section rounded up to 256 bytes; npts and nslots do not enter. */
int orbl_update_connections_workspace(int ntgt, int nkf, int npts, int nslots, int nconn, size_t* bytes);

/* ---- KeyFrame::SetBadFlag (src/KeyFrame.cc:460-553) with EraseConnection (:560-573), UpdateBestCovisibles (:172-193) and
 * MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:140-191, monocular) for a WHOLE list of keyframes in ONE call, with the exact
 * sequential semantics of calling it on each in turn.  Keyframes are 0..nkf-1, points 0..npts-1.
 *   targets, in call order: tgt_kf[t] in [0, nkf), distinct; tgt_flags[t] (nullable = all 0): bit 0 = id_ == 0, bit 1 = do_not_erase_ (the
 *     bits of cand_flags in orbl_keyframe_culling); tgt_mask[t] (nullable = all 1): 0 = SetBadFlag is not called on this target - the
 *     layout of culled[] from orbl_keyframe_culling, so the device entry can be enqueued directly behind the culling's with d_culled.
 *   keyframe tables: kf_bad[nkf] (IN/OUT), kf_parent[nkf] (IN/OUT, -1 = none), kf_rank[nkf] (nullable = index order): a permutation, the
 *     position under std::less<KeyFrame*>; kf_Tcw[nkf][12] row-major 3x4 (IN); child_off[nkf + 1] / child_kf[] = childrens_, rows in any
 *     order; conn_off / conn_kf / conn_w = connected_keyframe_weights_, any order inside a row, a row names a keyframe at most once and
 *     never itself; ord_off / ord_kf / ord_w = ordered_connected_keyframes_ / ordered_weights_ (the layouts
 *     orbl_essential_graph_assemble reads).  Ids are unique, so the id comparison at :516 is index equality: no id table enters.
 *   point tables, nullable AS A SET (without them step 2 is left out): kf_slot_off[nkf + 1] / kf_slot_pt[] (IN/OUT, -1 = null slot),
 *     pt_bad[npts], pt_nobs[npts], pt_ref_kf[npts] (IN/OUT), obs_off[npts + 1] / obs_kf[] / obs_slot[], each list in std::map order and
 *     naming a keyframe at most once, slot obs_slot[e] of keyframe obs_kf[e] holding the point; OUT obs_erased[nobs].  As in
 *     orbl_local_ba_apply every observation listed at entry is alive and every death of this call is written to obs_erased.
 * Per target t in order, B = tgt_kf[t]:
 *   0. mask 0: tgt_status = 3; bit 0: tgt_status = 1 (:463); bit 1: tgt_status = 2 (:465-468; setting do_to_be_erased_ stays with the
 *      caller).  Nothing changes in these cases.  Otherwise tgt_status = 0 and steps 1 to 5 run.
 *   1. (:471-476) for every k in B's conn row whose OWN conn row names B: that entry of k goes, and k's ordered list becomes ALL that is
 *      left of k's row by descending (weight, kf_rank) - the re-sort orbl_update_connections documents, which can make the list longer
 *      than it was.  A keyframe that names B while B does not name it keeps the entry and its list; one B names that does not name B is
 *      untouched.
 *   2. (:478-480, only with the point tables) for every non-null slot of B in slot order, point p: nothing when p has no alive
 *      observation by B (it turned bad already, or is listed twice).  Otherwise that observation dies and pt_nobs[p]--; pt_ref_kf[p] == B
 *      becomes the observer of p's first alive entry (it stays when none is left); pt_nobs[p] <= 2 turns p bad: every observation of it
 *      that is still alive dies and slot obs_slot[e] of its keyframe becomes -1.  B's own slots are not cleared.
 *   3. (:486-487) B's conn and ord rows become empty.
 *   4. (:490-544) P = kf_parent[B], candidates = {P}.  While B has children: over the children that are not bad NOW in ascending kf_rank,
 *      over each child's ordered list as it stands now in list order, every entry that is a candidate with w = its weight in the child's
 *      conn row (0 when absent) replaces the best when w is STRICTLY greater (the best starts at -1).  A best (child, entry):
 *      kf_parent[child] = entry, the child joins entry's children, leaves B's and joins the candidates.  None: stop.  Every child still
 *      in B's row, bad ones included, then gets kf_parent = P and joins P's children; it STAYS in B's row.
 *   5. (:544-552) B leaves P's children; tgt_Tcp[t] = Tcw[B] o Twc[P], the product of orbl_propagate_global_ba (FP64, no fused
 *      multiply-add, sums in index order); kf_bad[B] = 1; kf_parent[B] stays.
 * Outputs: tgt_status[ntgt]; tgt_Tcp[ntgt][12], zeros where the status is not 0; the in/out tables; the WHOLE new tables, which are
 * what the next entry reads: oconn_off[nkf + 1] / oconn_kf / oconn_w (each row in its input order with the removed entries closed up;
 * arrays of conn_off[nkf] entries always suffice), oord_off[nkf + 1] / oord_kf / oord_w of capacity cap_ord (an untouched row is
 * copied, a re-sorted one is the new list), ochild_off[nkf + 1] / ochild_kf of capacity cap_child, rows in ascending kf_rank; counts[6] =
 * {n_bad, n_conn_out, n_ord_out, n_child_out, n_adopted (children given a candidate as parent), n_fallback (children handed to P)}.
 * Every element inside the counts is written, nothing beyond a capacity; the outputs are the same bytes on every run.
 * OUT OF SCOPE, stays with the caller: map_->EraseKeyFrame, keyframe_database_->erase (orbv_db_erase), map_->EraseMapPoint for the
 * points that turned bad, do_to_be_erased_, LocalMapping::MapPointCulling's tests (its SetBadFlag calls: orbl_apply_map_edits, kind 3).
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for negative counts or
 * capacities, NULL where an array is needed, part of the point set without the rest, offsets that do not ascend from 0, indices out of
 * range, a kf_rank that is no permutation, a duplicate target, a status-0 target that is already bad or whose parent is -1 or itself
 * (the reference dereferences it), a conn or child row that names a keyframe twice or itself, an obs_slot outside its keyframe's slots
 * or whose slot does not hold the point, an observation list naming a keyframe twice; ORBHIP_ENODEV without a GPU; ORBHIP_ECAP, with
 * only counts[] (the wanted sizes) written and the in/out tables untouched, when a list does not fit.                              */
int orbl_set_bad_keyframes(int ntgt, const int32_t* tgt_kf, const uint8_t* tgt_flags, const uint8_t* tgt_mask, int nkf, uint8_t* kf_bad, int32_t* kf_parent,
                           const int32_t* kf_rank, const double* kf_Tcw, const int32_t* child_off, const int32_t* child_kf, const int32_t* conn_off,
                           const int32_t* conn_kf, const int32_t* conn_w, const int32_t* ord_off, const int32_t* ord_kf, const int32_t* ord_w, int npts,
                           const int32_t* kf_slot_off, int32_t* kf_slot_pt, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_ref_kf, const int32_t* obs_off,
                           const int32_t* obs_kf, const int32_t* obs_slot, uint8_t* obs_erased, int cap_ord, int cap_child, int32_t* tgt_status, double* tgt_Tcp,
                           int32_t* oconn_off, int32_t* oconn_kf, int32_t* oconn_w, int32_t* oord_off, int32_t* oord_kf, int32_t* oord_w, int32_t* ochild_off,
                           int32_t* ochild_kf, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation and no allocation inside (nchild = child_off[nkf], nconn =
 * conn_off[nkf], nord = ord_off[nkf], nslots = kf_slot_off[nkf], nobs = obs_off[npts] given by the caller; the point set is absent when
 * d_kf_slot_off is NULL).  d_counts[6] always holds the WANTED counts.  Counts, NULL pointers and alignment (4 bytes, 8 for the poses)
 * are checked on the host; the data is bounds-checked on the device and an entry out of range counts as ABSENT: a connection, list
 * entry, child, slot or observation that is not there, a target skipped with tgt_status = 4.  *d_status (nullable; zeroed first):
 * 1 = offsets; 2 = an index out of range or a kf_rank that is no permutation; 4 = a target skipped with tgt_status = 4 (out of range,
 * already bad, parent -1 / itself / out of range, or listed twice among the status-0 targets: the first instance counts); 8 = a conn
 * row naming itself, a child row naming itself or a keyframe twice (the repeat is absent); 16 / 32 = cap_ord / cap_child exceeded
 * (the elements below the capacity are still written, none beyond it).  PRECONDITIONS, not checked here: no conn row and no observation
 * list names a keyframe twice, and an observation's slot holds its point.  `d_workspace`: at least orbl_set_bad_keyframes_workspace(...)
 * bytes of device memory, 4-byte aligned, not shared with concurrent calls; it is cleared by every call, so calls may reuse it. */
int orbl_set_bad_keyframes_device(int ntgt, const int32_t* d_tgt_kf, const uint8_t* d_tgt_flags, const uint8_t* d_tgt_mask, int nkf, uint8_t* d_kf_bad,
                                  int32_t* d_kf_parent, const int32_t* d_kf_rank, const double* d_kf_Tcw, int nchild, const int32_t* d_child_off,
                                  const int32_t* d_child_kf, int nconn, const int32_t* d_conn_off, const int32_t* d_conn_kf, const int32_t* d_conn_w, int nord,
                                  const int32_t* d_ord_off, const int32_t* d_ord_kf, const int32_t* d_ord_w, int npts, int nslots, const int32_t* d_kf_slot_off,
                                  int32_t* d_kf_slot_pt, uint8_t* d_pt_bad, int32_t* d_pt_nobs, int32_t* d_pt_ref_kf, int nobs, const int32_t* d_obs_off,
                                  const int32_t* d_obs_kf, const int32_t* d_obs_slot, uint8_t* d_obs_erased, int cap_ord, int cap_child, int32_t* d_tgt_status,
                                  double* d_tgt_Tcp, int32_t* d_oconn_off, int32_t* d_oconn_kf, int32_t* d_oconn_w, int32_t* d_oord_off, int32_t* d_oord_kf,
                                  int32_t* d_oord_w, int32_t* d_ochild_off, int32_t* d_ochild_kf, int32_t* d_counts, uint32_t* d_status, void* d_workspace,
                                  void* stream);
/* *bytes = the workspace orbl_set_bad_keyframes_device needs (host arithmetic; nobs = 0 without the point set).  With R(x) = x rounded up
 * to a multiple of 256 and adds = ntgt * nkf (a turn hands each child of its target to one new row, and a row is a set):
 *   4 R(4 nkf) + R(4 nconn) + R(4) + R(nchild) + R(nobs)        cleared by every call: first turn, rank check, two stamp arrays per
 *                                                                 keyframe; the mutual turn per conn entry; one counter; one byte per
 *                                                                 child entry and per observation
 * + R(4 nkf) + R(4 ntgt)                                        the first erasing turn per keyframe, the tentative status per target
 * + 2 R(4 adds) + R(adds)                                       the new child memberships: parent, child, alive byte
 * + 2 R(4 nkf) + R(12 nkf) + R(4 (nchild + adds))               the current target's children, three row sizes, the gathered children */
int orbl_set_bad_keyframes_workspace(int ntgt, int nkf, int nchild, int nconn, int nobs, size_t* bytes);

/* ---- Map-point edits on the tables: an ORDERED list of MapPoint::AddObservation / Replace / SetBadFlag calls (src/MapPoint.cc:133-138,
 * :199-233, :174-191, monocular), as LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:141-152), CreateNewMapPoints (:380-385),
 * MapPointCulling (:167-194), ORBmatcher::Fuse (src/ORBmatcher.cc:746, :824-838; the Sim3 form :941-950), LoopClosing::CorrectLoop
 * (src/LoopClosing.cc:527-539) and SearchAndFuse (:615-621) make them, replayed in call order in ONE call that returns the WHOLE new
 * observation tables.  With nops = 0 it is the rebuild between two other table calls: every other entry only reports deaths in
 * obs_erased[] and requires its input lists alive.  Keyframes are 0..nkf-1, points 0..npts-1; a freshly created map point is a row the
 * caller appended with an empty list and pt_nobs = 0, a new keyframe a row with its slots.
 *   IN: kf_slot_off[nkf + 1]; kf_rank[nkf] (nullable = index order; a permutation: the position under std::less<KeyFrame*>);
 *     obs_off[npts + 1] / obs_kf[] / obs_slot[], a list naming a keyframe at most once, in any order; obs_dead[nobs] (nullable): an
 *     obs_erased[] of an earlier call - such entries are ABSENT (only their obs_kf must be a keyframe); kf_slot_level[nslots] and kf_slot_uv[nslots][2] (float), nullable as a pair.
 *   IN/OUT in place: kf_slot_pt[] (-1 = null); pt_bad[npts]; pt_nobs[npts] = Observations(), which is NOT the list length and is never
 *     reset, exactly as in the reference; pt_found[npts] / pt_visible[npts] (nullable as a pair); pt_replaced[npts] (nullable, -1 = none).
 *   The edits, in call order: op_kind[nops], op_pt, op_arg, op_kf, op_slot.
 * The primitives:
 *   AddObs(p, K, s)  false when p's list names K; otherwise the list gains (K, s), pt_nobs[p]++, true.
 *   Replace(a, b)    nothing when a == b.  Otherwise a's list is taken and emptied, pt_bad[a] = 1, pt_replaced[a] = b; for each taken
 *                    (k, s): when b's list does not name k, slot (k, s) becomes b and AddObs(b, k, s) runs, otherwise slot (k, s)
 *                    becomes -1; pt_found[b] += pt_found[a], pt_visible[b] += pt_visible[a] (a's counters are NOT cleared: a second
 *                    Replace of the same a adds them again, as SearchAndFuse can); b is TOUCHED (ComputeDistinctiveDescriptors, :230).
 *                    No bad-flag test on a or on b.
 *   SetBad(p)        pt_bad[p] = 1, p's list is emptied, every slot it named becomes -1.
 * Kinds and op_status:
 *   0 NOP                                  a row the caller masked out.  Status 0.
 *   1 ADD(p = op_pt, K, s; op_arg bit 0 = touch)   ok = AddObs(p, K, s); slot (K, s) becomes p UNCONDITIONALLY (KeyFrame::AddMapPoint;
 *                                          LoopClosing.cc:534-535 writes it even when p is observed elsewhere in K); with bit 0 p is
 *                                          touched.  Status 5 when ok, 6 when not.
 *   2 REPLACE(a = op_pt, b = op_arg)       Replace(a, b).  Status 8, or 1 when a == b.
 *   3 SET_BAD(p)                           SetBad(p): the mutation of MapPointCulling; its found-ratio and age tests stay with the
 *                                          caller.  Status 9.
 *   4 FUSE(p, K, s)                        skipped (1) when pt_bad[p] or p's list names K.  Otherwise q = slot (K, s): q >= 0 and bad:
 *                                          nothing (2); q >= 0 and not bad: pt_nobs[q] > pt_nobs[p] ? Replace(p, q) (3) : Replace(q, p)
 *                                          (4; a tie replaces q); q < 0: ADD without touch (5; 6 cannot occur after the skip test).
 *   5 FIND_OR_ADD(p, K, s)                 q = slot (K, s): q >= 0 and bad: nothing (2); q >= 0 and alive: op_found = q (7); q < 0: ADD
 *                                          without touch (5 or 6).  No skip test: the caller filters isBad() || spAlreadyFound (:872)
 *                                          before the call - exact, because a Sim3 Fuse changes no bad flag and the set is a snapshot.
 *   6 REPLACE_FOUND(j = op_arg, b = op_pt) j < i names a kind-5 op: a = op_found[j]; -1: skipped (1); otherwise Replace(a, b) (8, or 1
 *                                          when a == b).
 *   op_found[i] = the point a kind-4 or kind-5 op met ALIVE in its slot, else -1.
 * Outputs: op_status[nops], op_found[nops]; pt_touched[npts] (uint8, every element written); the in/out tables; the whole new tables,
 * each list in ascending kf_rank (the std::map order every other entry wants): oobs_off[npts + 1], oobs_kf, oobs_slot, oobs_src
 * (nullable: the input index e of a surviving or moved observation, nobs + i for the one op i created) and, with the kf_slot_level pair,
 * oobs_level / oobs_uv gathered from (keyframe, slot) - of capacity cap_obs; nobs + nops always suffices.  counts[8] = {n_obs_out,
 * n_obs_added (observations created: the ops that ended with status 5), n_replace (Replace calls that ran), n_set_bad, n_fused (ops of
 * kinds 4 and 5 with status 2, 3, 4, 5 or 7: the nFused both Fuse functions return, with ONE exception - the Sim3 form increments
 * nFused for a row whose AddObservation is refused as well (kind 5, status 6), which is not counted here; add the ops with that
 * status for the reference's number), n_touched, n_late_adds, 0}.
 * n_late_adds = the points that were touched and received an observation created by an op AFTER their last touch.  The caller recomputes
 * descriptors after the call: one orbl_update_map_points(_device) on the pt_touched points equals the reference's in-loop
 * ComputeDistinctiveDescriptors exactly when this count is 0.  It is 0 for any single-keyframe Fuse, for the CorrectLoop loop and for a
 * SearchAndFuse keyframe, because after its touch a point is in the keyframe or bad: Replace(x, b) runs only when b is in the slot or
 * takes it over from x, so b's list names K from then on and FUSE skips it (1), while x is bad and is skipped too; FIND_OR_ADD never
 * touches, and the REPLACE_FOUND ops that do come after every add of their keyframe.
 * Every element inside a count is written, nothing beyond a count or a capacity; the outputs are the same bytes on every run.
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for negative counts or
 * capacities, NULL where an array is needed or half of a nullable pair, offsets that do not ascend from 0, an index, slot or kind out of
 * range, a kf_rank that is no permutation, a list naming a keyframe twice, an alive observation whose slot does not hold its point, the
 * op_arg of a kind-6 op not in [0, i) or not naming a kind-5 op; ORBHIP_ENODEV without a GPU (there is no CPU fallback); ORBHIP_ECAP, with
 * only counts[] written and the in/out tables untouched, when cap_obs is too small.                                                   */
int orbl_apply_map_edits(int nops, const int32_t* op_kind, const int32_t* op_pt, const int32_t* op_arg, const int32_t* op_kf, const int32_t* op_slot, int nkf,
                         const int32_t* kf_slot_off, const int32_t* kf_rank, int32_t* kf_slot_pt, const int32_t* kf_slot_level, const float* kf_slot_uv, int npts,
                         uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_found, int32_t* pt_visible, int32_t* pt_replaced, const int32_t* obs_off,
                         const int32_t* obs_kf, const int32_t* obs_slot, const uint8_t* obs_dead, int cap_obs, int32_t* op_status, int32_t* op_found,
                         uint8_t* pt_touched, int32_t* oobs_off, int32_t* oobs_kf, int32_t* oobs_slot, int32_t* oobs_src, int32_t* oobs_level, float* oobs_uv,
                         int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`: no synchronisation, no allocation and no host read of the data (nslots =
 * kf_slot_off[nkf], nobs = obs_off[npts] given by the caller; d_kf_slot_off and d_obs_off are needed even without rows: one 0).
 * d_counts[8] always holds the WANTED counts.  Counts, NULL pointers and alignment (4 bytes) are checked on the host; the data is
 * bounds-checked on the device: an op out of range is ABSENT (op_status 10, op_found -1), an observation out of range is absent, a slot
 * holding a point out of range counts as null.  *d_status (nullable; zeroed first): 1 = offsets; 2 = a keyframe out of range or a
 * kf_rank that is no permutation; 4 = a point out of range; 8 = a slot its keyframe does not have, a kind out of range or a kind-6 op
 * whose op_arg names no earlier kind-5 op; 16 = cap_obs exceeded (the elements below the capacity are still written, none beyond it).
 * PRECONDITIONS, not checked here: no list names a keyframe twice, and an alive observation's slot holds its point.  `d_workspace`: at
 * least orbl_apply_map_edits_workspace(...) bytes of device memory, 4-byte aligned, not shared with concurrent calls; it is cleared by
 * every call, so calls may reuse it.                                                                                                  */
int orbl_apply_map_edits_device(int nops, const int32_t* d_op_kind, const int32_t* d_op_pt, const int32_t* d_op_arg, const int32_t* d_op_kf,
                                const int32_t* d_op_slot, int nkf, const int32_t* d_kf_slot_off, const int32_t* d_kf_rank, int nslots, int32_t* d_kf_slot_pt,
                                const int32_t* d_kf_slot_level, const float* d_kf_slot_uv, int npts, uint8_t* d_pt_bad, int32_t* d_pt_nobs, int32_t* d_pt_found,
                                int32_t* d_pt_visible, int32_t* d_pt_replaced, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                const int32_t* d_obs_slot, const uint8_t* d_obs_dead, int cap_obs, int32_t* d_op_status, int32_t* d_op_found, uint8_t* d_pt_touched,
                                int32_t* d_oobs_off, int32_t* d_oobs_kf, int32_t* d_oobs_slot, int32_t* d_oobs_src, int32_t* d_oobs_level, float* d_oobs_uv,
                                int32_t* d_counts, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_apply_map_edits_device needs (host arithmetic; nslots does not enter).  With R(x) = x rounded up to a
 * multiple of 256, ents = nobs + nops and blocks = ceil(npts / 256):
 *   2 R(npts) + R(4 nkf) + R(8)                 cleared by every call: a point's list was emptied, it has a late add; the rank check;
 *                                               two counters
 * + R(4 npts) + R(4 ents) + R(nobs)             the head of a point's chain of received entries, the chain links, one byte per input
 *                                               observation that is there
 * + 2 R(4 npts) + R(4 (blocks + 1)) + R(4 ents) the new list lengths and their scan, the workgroup sums, the gathered entries         */
int orbl_apply_map_edits_workspace(int nops, int nkf, int npts, int nslots, int nobs, size_t* bytes);

/* ---- LocalMapping::SearchInNeighbors on the resident tables (src/LocalMapping.cc:398-488): the four pieces a caller whose map tables
 * stay on the device lacked between orbl_apply_map_edits and orbl_update_map_points.  The exact loop is, per target keyframe in list
 * order: orbl_fuse_rows_device (the descriptors as they stand) -> orbl_apply_map_edits_device (the FUSE op tests the bad flags,
 * IsInKeyFrame, Observations() and the slots at each row's own turn) -> orbl_update_map_points_on_tables_device(ORBL_MP_DESC,
 * pt_touched).  Inside ONE keyframe's Fuse every search uses the descriptors held at entry (n_late_adds == 0 above), and across
 * keyframes nothing else the projection reads changes: Replace and AddObservation leave position, normal and the depth range alone.
 * The points of the first loop are a snapshot of the current keyframe's slot row taken BEFORE the loop (:435).  INTEGRATION.md section 4
 * has the call sequence.  Each entry has a host form (host pointers, synchronous, one packed upload and one download; ORBHIP_EINVAL
 * before any device work, ORBHIP_ENODEV without a GPU: no CPU fallback), a _device form (device pointers, enqueued on `stream`: no
 * synchronisation, no allocation, no host read of the data; counts, NULL pointers and alignment checked on the host, the data
 * bounds-checked on the device - an entry out of range counts as absent and raises a bit of *d_status, nullable and zeroed first:
 * 1 = offsets, 2 = a keyframe out of range, 4 = a point out of range, 8 = a level out of range, 16 = a capacity exceeded, 32 = a slot
 * its keyframe does not have) and a _workspace form (host arithmetic; R(x) = x rounded up to a multiple of 256).                      */

/* The target keyframes (:400-431).  kf_bad[nkf] (nullable = none); every keyframe's ordered_connected_keyframes_ as ord_off[nkf + 1] /
 * ord_kf[]; kf_fuse_target[nkf] (IN/OUT), the fuse_target_for_keyframe_ stamps.  Literally: for each of the first nn entries n of
 * cur_kf's list, in order: skipped when kf_bad[n] or kf_fuse_target[n] == cur_id; otherwise n is pushed and stamped, and each of the
 * first nn2 entries k2 of n's list is pushed WITHOUT a stamp unless kf_bad[k2], kf_fuse_target[k2] == cur_id or k2 == cur_kf.  The list
 * therefore names a keyframe twice when a second neighbour is reached twice or is itself a later first neighbour, as the reference's
 * does.  The reference calls it with nn = 20, nn2 = 5; at most nn (1 + nn2) entries result.  tgt_kf[cap_tgt]; counts[2] = {the wanted
 * number of targets, the first neighbours among them}.  Host form: cur_kf and every ord_kf entry must be a keyframe (EINVAL);
 * ORBHIP_ECAP with only counts[] written when cap_tgt is too small.  Device form: an entry that is no keyframe is skipped (bit 2),
 * nothing is written beyond cap_tgt (bit 16).  One wave; the workspace is 0 bytes and may be NULL.                                    */
int orbl_fuse_targets(int cur_kf, int cur_id, int nkf, const uint8_t* kf_bad, const int32_t* ord_off, const int32_t* ord_kf, int32_t* kf_fuse_target, int nn, int nn2,
                      int cap_tgt, int32_t* tgt_kf, int32_t* counts);
int orbl_fuse_targets_device(int cur_kf, int cur_id, int nkf, const uint8_t* d_kf_bad, int nord, const int32_t* d_ord_off, const int32_t* d_ord_kf,
                             int32_t* d_kf_fuse_target, int nn, int nn2, int cap_tgt, int32_t* d_tgt_kf, int32_t* d_counts, uint32_t* d_status, void* d_workspace,
                             void* stream);
int orbl_fuse_targets_workspace(int nkf, size_t* bytes);

/* The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:739-824) for ONE keyframe and a list of points, everything
 * read from the tables, edit rows out.  The device form names the keyframe by a device pointer d_kf to its index, so a chain walks
 * d_tgt_kf + t without a host copy of the target list.  pts[n], -1 = null.
 *   Keyframe tables: kf_Tcw[nkf][12], kf_center[nkf][3] (double); kf_K4[nkf][4] {fx, fy, cx, cy} and kf_bounds[nkf][4] {min_x_, max_x_,
 *   min_y_, max_y_} (float); kf_slot_off[nkf + 1]; kf_slot_uv[nslots][2] (float, the undistorted keypoints), kf_slot_level[nslots],
 *   kf_slot_desc[nslots][32], the keyframe's descriptor rows.
 *   Point tables: pt_Xw[npts][3], pt_normal[npts][3] (double); pt_min_dist[npts], pt_max_dist[npts] (float, raw: the 0.8 / 1.2 factors of
 *   Get{Min,Max}DistanceInvariance are applied inside); pt_desc[npts][32].
 *   scale_factors[n_levels], inv_level_sigma2[n_levels], log_scale_factor, th (the reference's default: 3.0).
 * The arithmetic is the reference's float / double mix: p3Dc = Rcw p + tcw in double, each row (r0 x + r1 y) + r2 z, then + t; p3Dc[2]
 * < 0 rejects; invz = (float)(1 / z), x = (float)(p3Dc[0] invz), u = fx x + cx in float; IsInImage is u >= min_x && u < max_x && v >=
 * min_y && v < max_y; dist3D = (float)|PO| with PO = p - Ow; dist3D < 0.8f min or > 1.2f max rejects; PO.Pn < 0.5 dist3D in double
 * rejects; level = ceilf(logf(max / dist3D) / log_scale_factor) clamped to [0, n_levels - 1].  Then KeyFrame::GetFeaturesInArea(u, v,
 * th scale_factors[level]) (src/KeyFrame.cc:575-622), the level window [level - 1, level] and e2 inv_level_sigma2[lvl] > 5.99.  The
 * least Hamming distance wins, the FIRST of equal ones in GetFeaturesInArea's output order: cells ix-major then iy, index order inside
 * a cell.  DEPARTURE in form only: no grid table is read - a keypoint's own cell is Frame::PosInGrid (src/Frame.cc:309-320) of its
 * position, which is how the reference's grid was filled, so the candidate list and its order are the same by construction.
 * Row i, in orbl_apply_map_edits' layout: NOP (kind 0, op_pt = the point or -1, op_arg 0, op_kf = the keyframe, op_slot -1) for a
 * null point, a failed gate, no candidate or a best distance > TH_LOW (50); otherwise FUSE (kind 4, op_pt, op_arg 0, op_kf, op_slot =
 * the best keypoint) - whatever the point's bad flag or IsInKeyFrame is: the replay's skip test decides that at the right moment.
 * Nullable outputs: best_idx[n] (-1 = none), best_dist[n] (256 = none), q_uv[n][2] and q_level[n] (-1 = a gate failed; then q_uv = 0):
 * what orbl_fuse_batch takes and returns.  Every element is written; the outputs are the same bytes on every run.
 * Host form: kf must be a keyframe, pts entries points or -1, the keyframe's kf_slot_level entries levels (EINVAL).  Device form: a
 * point out of range is a NOP (bit 4), a keyframe out of range makes every row a NOP (bit 2), a keypoint with a negative level that the
 * window would admit is skipped (bit 8).  Descriptor tables 4-byte aligned.  One wave per point; the workspace is 0 bytes, may be NULL. */
int orbl_fuse_rows(int kf, int n, const int32_t* pts, int nkf, const double* kf_Tcw, const double* kf_center, const float* kf_K4, const float* kf_bounds,
                   const int32_t* kf_slot_off, const float* kf_slot_uv, const int32_t* kf_slot_level, const uint8_t* kf_slot_desc, int npts, const double* pt_Xw,
                   const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist, const uint8_t* pt_desc, const float* scale_factors,
                   const float* inv_level_sigma2, float log_scale_factor, int n_levels, float th, int32_t* op_kind, int32_t* op_pt, int32_t* op_arg, int32_t* op_kf,
                   int32_t* op_slot, int32_t* best_idx, int32_t* best_dist, float* q_uv, int32_t* q_level);
int orbl_fuse_rows_device(const int32_t* d_kf, int n, const int32_t* d_pts, int nkf, const double* d_kf_Tcw, const double* d_kf_center, const float* d_kf_K4,
                          const float* d_kf_bounds, const int32_t* d_kf_slot_off, int nslots, const float* d_kf_slot_uv, const int32_t* d_kf_slot_level,
                          const uint8_t* d_kf_slot_desc, int npts, const double* d_pt_Xw, const double* d_pt_normal, const float* d_pt_min_dist,
                          const float* d_pt_max_dist, const uint8_t* d_pt_desc, const float* d_scale_factors, const float* d_inv_level_sigma2, float log_scale_factor,
                          int n_levels, float th, int32_t* d_op_kind, int32_t* d_op_pt, int32_t* d_op_arg, int32_t* d_op_kf, int32_t* d_op_slot, int32_t* d_best_idx,
                          int32_t* d_best_dist, float* d_q_uv, int32_t* d_q_level, uint32_t* d_status, void* d_workspace, void* stream);
int orbl_fuse_rows_workspace(int n, size_t* bytes);

/* The candidates of the second direction (:445-470): tgt_kf[n_tgt], the target list with its duplicates; kf_slot_off / kf_slot_pt;
 * pt_bad[npts]; pt_fuse_cand[npts] (IN/OUT), the fuse_candidate_for_keyframe stamps.  cand_pt[cap_cand] = the first occurrence of every
 * point that is non-null, not bad and not stamped cur_id at entry, the targets walked in list order and a target's slots in slot
 * order; every emitted point ends stamped.  counts[2] = {the wanted number of candidates, n_tgt}.  No atomic decides a position (a
 * minimum of (list position, slot) per point, then ordered scans): the outputs are the same bytes on every run.  Host form: EINVAL for
 * a target that is no keyframe or a slot holding neither a point nor -1; ORBHIP_ECAP with only counts[] written when cap_cand is too
 * small.  Device form: such targets and slots are skipped (bits 2, 4); nothing is written beyond cap_cand (bit 16) and the points
 * beyond it stay unstamped.  n_tgt <= 2^24.  Workspace, 8-byte aligned: R(8 npts) + R(4 (n_tgt + 1)).                                 */
int orbl_fuse_candidates(int n_tgt, const int32_t* tgt_kf, int nkf, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const uint8_t* pt_bad,
                         int32_t* pt_fuse_cand, int cur_id, int cap_cand, int32_t* cand_pt, int32_t* counts);
int orbl_fuse_candidates_device(int n_tgt, const int32_t* d_tgt_kf, int nkf, const int32_t* d_kf_slot_off, int nslots, const int32_t* d_kf_slot_pt, int npts,
                                const uint8_t* d_pt_bad, int32_t* d_pt_fuse_cand, int cur_id, int cap_cand, int32_t* d_cand_pt, int32_t* d_counts, uint32_t* d_status,
                                void* d_workspace, void* stream);
int orbl_fuse_candidates_workspace(int n_tgt, int npts, size_t* bytes);

/* MapPoint::ComputeDistinctiveDescriptors and / or UpdateNormalAndDepth (`what` as in orbl_update_map_points) for the points a mask
 * selects, read straight from the tables and written IN PLACE.  The selection: pt_mask[npts] (nullable; orbl_apply_map_edits'
 * pt_touched) and / or the non-null slots of keyframe mask_kf (-1 = none; :474-485) - at least one of the two.  What
 * orbl_update_map_points takes per observation is gathered first: the descriptor of observation e from kf_slot_desc through (obs_kf,
 * obs_slot), obs_kf_good from kf_bad (nullable = none), and per point the reference level - the kf_slot_level of the observation in
 * pt_ref_kf[p], or of that keyframe's keypoint 0 when the list does not name it (the rule stated above).  The rest is
 * orbl_update_map_points' own kernels, so the results are bit-identical to that entry on the same lists: pt_desc[npts][32],
 * pt_normal[npts][3], pt_min_dist[npts], pt_max_dist[npts]; bad points, unselected points and empty lists are left alone.  Nullable
 * outputs: best_obs[npts] (the list position of the chosen descriptor, -1 = unchanged; written for every point with ORBL_MP_DESC),
 * nd_written[npts] (with ORBL_MP_NORMAL_DEPTH).  The lists must be alive and in the order the reference walks them (ascending kf_rank:
 * the tables orbl_apply_map_edits returns).  kf_slot_desc is needed whatever `what` is; kf_center, kf_slot_level, pt_Xw, pt_ref_kf,
 * scale_factors only for ORBL_MP_NORMAL_DEPTH; kf_slot_pt only with mask_kf.  Host form: EINVAL for an observation that names no
 * keyframe or no slot of it, a pt_ref_kf that is neither a keyframe nor -1, a level out of range.  Device form: such an observation is
 * absent (bits 2, 32).  Workspace, 16-byte aligned: R(npts) cleared by every call + R(npts) + 2 R(4 npts) + R(npts) + R(8 npts) +
 * R(nobs) + R(32 nobs) + R(32 + 20 npts), the last one orbl_update_map_points' own.                                                   */
int orbl_update_map_points_on_tables(int what, const uint8_t* pt_mask, int mask_kf, int nkf, const uint8_t* kf_bad, const double* kf_center, const int32_t* kf_slot_off,
                                     const int32_t* kf_slot_pt, const int32_t* kf_slot_level, const uint8_t* kf_slot_desc, int npts, const uint8_t* pt_bad,
                                     const double* pt_Xw, const int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot,
                                     const float* scale_factors, int n_levels, uint8_t* pt_desc, double* pt_normal, float* pt_min_dist, float* pt_max_dist,
                                     int32_t* best_obs, uint8_t* nd_written);
int orbl_update_map_points_on_tables_device(int what, const uint8_t* d_pt_mask, int mask_kf, int nkf, const uint8_t* d_kf_bad, const double* d_kf_center,
                                            const int32_t* d_kf_slot_off, int nslots, const int32_t* d_kf_slot_pt, const int32_t* d_kf_slot_level,
                                            const uint8_t* d_kf_slot_desc, int npts, const uint8_t* d_pt_bad, const double* d_pt_Xw, const int32_t* d_pt_ref_kf,
                                            int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf, const int32_t* d_obs_slot, const float* d_scale_factors,
                                            int n_levels, uint8_t* d_pt_desc, double* d_pt_normal, float* d_pt_min_dist, float* d_pt_max_dist, int32_t* d_best_obs,
                                            uint8_t* d_nd_written, uint32_t* d_status, void* d_workspace, void* stream);
int orbl_update_map_points_on_tables_workspace(int npts, int nobs, size_t* bytes);

/* ---- LoopClosing::ComputeSim3, its front (src/LoopClosing.cc:250-277), on the resident tables for EVERY candidate in one call: per
 * candidate ORBmatcher::SearchByBoW(current keyframe, candidate) (src/ORBmatcher.cc:470-580), the `nmatches < min_matches` gate (:265)
 * and what Sim3Solver's constructor builds (src/Sim3Solver.cc:73-109).  The outputs are the d_X1c / d_X2c / d_max_err1 / d_max_err2 /
 * d_off / d_K1 / d_K2 arguments of orbt_sim3_iterate_batch_device (n_total = cap_rows) and the P3D1c / P3D2c / offsets of
 * ba_optimize_sim3_batch_device: a caller reads off[] alone (it needs every N to draw the sets) and goes on.  The three forms follow
 * the conventions of the SearchInNeighbors entries above (host form / _device form with *d_status / _workspace form).
 * Inputs, all read from the tables:
 *   cur_kf; cand_kf[n_cand], n_cand in [1, 1024] - a candidate may be cur_kf or appear twice, every row is computed on its own;
 *   kf_bad[nkf] (nullable = none), kf_Tcw[nkf][12], kf_K4[nkf][4] = (fx, fy, cx, cy);
 *   kf_slot_off[nkf + 1] over kf_slot_pt[] (map_points_, -1 = none), kf_slot_level[] (undistort_keypoints_[i].octave),
 *     kf_slot_angle[] (undistort_keypoints_[i].angle, float) and kf_slot_desc[][32].  A keyframe that takes part has at most 32768
 *     slots (ORBT_SIM3_MAX_N);
 *   every keyframe's feature_vector_ in orbv_transform's layout, concatenated: kf_fv_off[nkf + 1] over fv_node[] (ascending inside a
 *     keyframe), fv_ent_off[nfv + 1] over fv_ent[] (the keypoint's index inside its keyframe, in list order).  A keyframe's feature
 *     vector names a keypoint at most once, as DBoW2 builds it;
 *   pt_bad[npts], pt_Xw[npts][3]; obs_off[npts + 1] over obs_kf[] / obs_slot[] (observations_);
 *   level_sigma2[n_levels] (level_sigma2s_: one extractor, one table); nnratio (the reference: 0.75), check_ori (1), min_matches (20);
 *   cap1: the row stride of match12, at least the current keyframe's slot count, at most 32768; cap_rows: the rows the packed outputs
 *     hold, at most 32768 n_cand.
 * Per candidate c, literally:
 *   1. A candidate whose keyframe is bad is not searched (:257-260): cand_status 1.
 *   2. SearchByBoW: the node merge of :498-560.  A feature of either side takes part when its slot holds a point that is not pt_bad.
 *      Inside a node the current keyframe's entries, in list order, each take the closest entry of the candidate's list that no earlier
 *      entry took (vbMatched2); of equal distances the first in list order (strict <); bestDist2 is the second smallest, an equal
 *      distance counted, both from 256.  Accepted iff bestDist1 < 50 and (float)bestDist1 < nnratio * (float)bestDist2.  With check_ori
 *      the bin of rot = angle1 - angle2 (+ 360 when negative), round(rot * (1.0f / 30)), 30 -> 0, and after ComputeThreeMaxima the
 *      matches of the other bins are cleared - their vbMatched2 stayed set during the search, as in the reference.
 *   3. nmatches < min_matches discards the candidate: cand_status 2.
 *   4. Otherwise (cand_status 0) the constructor's loop, i1 ascending.  Row i1 is skipped when match12[i1] < 0, when slot i1 of the
 *      current keyframe holds no point, when either point is bad, or when GetIndexInKeyFrame is negative on either side.
 *      GetIndexInKeyFrame(point, keyframe) is obs_slot of the FIRST entry of the point's observation list that names the keyframe, -1
 *      when none does - not the slot the point was found in.  The octave is kf_slot_level at THAT index, max_err = (float)(size_t)
 *      (9.210 * (double)level_sigma2[octave]), and X = ((R(i,0) x + R(i,1) y) + R(i,2) z) + t(i) in double without fused multiply-add.
 *      A kept candidate may end with fewer than min_matches rows: the reference builds its solver and iterate answers TOO_FEW.
 * Outputs, every element written on every call:
 *   match12[n_cand][cap1]: the candidate keyframe's slot or -1, after the rotation check (map_point_matches_vector[i], as slots);
 *   nmatches[n_cand] (0 for cand_status 1); cand_status[n_cand]; K1[n_cand][4], K2[n_cand][4] = kf_K4 of the current keyframe and of the
 *     candidate (K2: zeros for cand_status 1; K1: zeros in the device form when the current keyframe is not usable);
 *   off[n_cand + 1]: the rows of candidate c are [off[c], off[c + 1]), empty for a discarded one;
 *   X1c, X2c[cap_rows][3]; max_err1, max_err2[cap_rows]; row_i1 (matched_indices_1_), row_pt1, row_pt2[cap_rows] (the points); rows
 *     behind the last one are zeros and -1;
 *   counts[2] = {rows wanted, candidates kept}.
 * No atomic decides a position: the same bytes on every run.
 * Host form: ORBHIP_EINVAL for anything the tables must not hold (an index out of range, offsets that decrease, fv_node not ascending, a
 * keypoint named twice, more than 32768 slots in a keyframe that takes part); ORBHIP_ECAP with only counts[] written when cap_rows is
 * too small (counts[0] = the rows wanted) or cap1 is below the current keyframe's slot count (counts = {0, 0}, the message names it).
 * Device form: an entry out of range counts as absent - a candidate that is no keyframe as a bad one (bit 2), a slot point that is no
 * point as none (bit 4), an fv_ent or obs_slot its keyframe does not have as missing (bit 32), a level out of range as no row (bit 8),
 * unusable offsets as an empty list (bit 1).  Bit 16: a keyframe that takes part has more than 32768 slots (it counts as bad), the
 * current keyframe has more than cap1 (nothing is searched), or more than cap_rows rows were wanted - off[] and counts[] then state
 * what was wanted and nothing is written beyond cap_rows.
 * Workspace, with R(x) = x rounded up to a multiple of 256: R(128 n_cand) (the rotation histograms, cleared by every call)
 * + R(n_cand cap1) (the bins) + 2 R(4 n_cand cap1) (the rows' keypoint indices) + R(4 (n_cand + 1)) (the row counts and their scan).   */
int orbl_loop_sim3_candidates(int cur_kf, int n_cand, const int32_t* cand_kf, int nkf, const uint8_t* kf_bad, const double* kf_Tcw, const float* kf_K4,
                              const int32_t* kf_slot_off, const int32_t* kf_slot_pt, const int32_t* kf_slot_level, const float* kf_slot_angle,
                              const uint8_t* kf_slot_desc, const int32_t* kf_fv_off, const uint32_t* fv_node, const int32_t* fv_ent_off, const int32_t* fv_ent, int npts,
                              const uint8_t* pt_bad, const double* pt_Xw, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_slot,
                              const float* level_sigma2, int n_levels, float nnratio, int check_ori, int min_matches, int cap1, int cap_rows, int32_t* match12,
                              int32_t* nmatches, int32_t* cand_status, float* K1, float* K2, int32_t* off, double* X1c, double* X2c, float* max_err1, float* max_err2,
                              int32_t* row_i1, int32_t* row_pt1, int32_t* row_pt2, int32_t* counts);
int orbl_loop_sim3_candidates_device(int cur_kf, int n_cand, const int32_t* d_cand_kf, int nkf, const uint8_t* d_kf_bad, const double* d_kf_Tcw, const float* d_kf_K4,
                                     int nslots, const int32_t* d_kf_slot_off, const int32_t* d_kf_slot_pt, const int32_t* d_kf_slot_level,
                                     const float* d_kf_slot_angle, const uint8_t* d_kf_slot_desc, int nfv, const int32_t* d_kf_fv_off, const uint32_t* d_fv_node,
                                     int nent, const int32_t* d_fv_ent_off, const int32_t* d_fv_ent, int npts, const uint8_t* d_pt_bad, const double* d_pt_Xw,
                                     int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf, const int32_t* d_obs_slot, const float* d_level_sigma2,
                                     int n_levels, float nnratio, int check_ori, int min_matches, int cap1, int cap_rows, int32_t* d_match12, int32_t* d_nmatches,
                                     int32_t* d_cand_status, float* d_K1, float* d_K2, int32_t* d_off, double* d_X1c, double* d_X2c, float* d_max_err1,
                                     float* d_max_err2, int32_t* d_row_i1, int32_t* d_row_pt1, int32_t* d_row_pt2, int32_t* d_counts, uint32_t* d_status,
                                     void* d_workspace, void* stream);
int orbl_loop_sim3_candidates_workspace(int n_cand, int cap1, size_t* bytes);

/* ---- LoopClosing::CorrectLoop, the part that moves the map (src/LoopClosing.cc:437-523): the corrected and non-corrected Sim3 of the
 * current keyframe's covisibility group, the correction of every map point those keyframes hold, UpdateNormalAndDepth of each moved
 * point, SetPose([R | t/s]) of each keyframe - with the exact semantics of the sequential loop.  Keyframes are 0..nkf-1, points 0..npts-1.
 *   kf_Tcw[nkf][12] (row-major 3x4, IN/OUT), kf_center[nkf][3] (nullable, IN/OUT): only the rows of the group are rewritten.
 *   conn_kf[nconn] = current_connected_keyframes_: distinct, the LAST entry is the current keyframe, nconn >= 1.
 *   conn_rank[nconn] (nullable = list order): a permutation, the keyframe's position under std::less<KeyFrame*> - the iteration order
 *     of sophus_corrected_sim3.   Scw[7]: Sophus storage [qx,qy,qz,qw, tx,ty,tz], |q|^2 = scale.
 *   slot_off[nconn + 1] / slot_pt[]: CSR of GetMapPointMatches() per connected keyframe: a point index or -1.
 *   X[npts][3] (IN/OUT); pt_bad[npts] (nullable); pt_done[npts] (nullable) = corrected_by_keyframe_ == current_keyframe_->id_ at entry.
 *   For the normals, as in orbl_update_map_points: obs_off[npts + 1] / obs_kf[] in the point's std::map order, ref_kf[npts],
 *     ref_level[npts], scale_factors[n_levels] - all nullable AS A SET (with normal, min_max, nd_written): then no normals are computed.
 *     With them kf_center is needed.
 * With A o B the product of two such matrices as 4x4 ones (last row 0 0 0 1), every sum in index order k = 0..3, and Twc what
 * KeyFrame::SetPose stores (Rwc = Rcw^T, Ow = -(Rwc tcw), each dot product (a0 b0 + a1 b1) + a2 b2):
 *   non_corrected[c] = Sim3(Tcw of conn_kf[c]): the matrix -> quaternion branches of ba_matrix4d_to_pose7, un-normalised, scale 1.
 *   corrected[last] = Scw; corrected[c] = ba_sim3_mul(Sim3(Tcw[c] o Twc[current]), Scw) otherwise.
 *   owner of p = the connected keyframe of lowest conn_rank that lists p; only points that are neither bad nor done take part.
 *   X[p] <- corrected[o]^-1 * (non_corrected[o] * X[p]) for the owner o;  pt_owner[p] = its keyframe index, or -1 (every element written):
 *     the caller sets corrected_by_keyframe_ and corrected_reference_ from it.
 *   new pose of conn_kf[c] = [R | t/s] of corrected[c] (the arithmetic of ba_essential_graph_correct); new centre = -(R^T t/s).
 *   normal / min_max / nd_written of every MOVED point as orbl_update_map_points computes them from the new position, where the centre
 *     of an observing (or the reference) keyframe k is its NEW centre when k is in the group and conn_rank(k) < conn_rank(owner), strictly -
 *     SetPose (:519) follows a keyframe's own points - and its centre at entry otherwise.  Rows of points that did not move are untouched.
 *   counts[2] = {n_moved, n_contested (moved points listed by two or more connected keyframes)}.
 * corrected[nconn][7] / non_corrected[nconn][7] are the two KeyFrameAndSim3 maps OptimizeEssentialGraph and SearchAndFuse take.  The
 * per-keyframe UpdateConnections() at :522 reads nothing this call writes: run orbl_update_connections on the list in conn_rank order
 * afterwards.  Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, NULLs,
 * offsets that do not ascend from 0, indices out of range, a duplicate in conn_kf, a conn_rank that is not a permutation, a level
 * outside [0, n_levels) or n_levels outside [1, 64], an Scw that is not finite or has |q|^2 = 0; ORBHIP_ENODEV without a GPU.          */
int orbl_correct_loop(int nkf, double* kf_Tcw, double* kf_center, int nconn, const int32_t* conn_kf, const int32_t* conn_rank, const double* Scw,
                      const int32_t* slot_off, const int32_t* slot_pt, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_done, const int32_t* obs_off,
                      const int32_t* obs_kf, const int32_t* ref_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, double* corrected,
                      double* non_corrected, int32_t* pt_owner, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nslots = slot_off[nconn], nobs = obs_off[npts] given by
 * the caller).  Counts, NULL pointers and alignment (8 bytes for the 64-bit arrays and the workspace, 4 for the 32-bit ones) are checked
 * on the host; the data is bounds-checked on the device: an entry out of range counts as ABSENT - a connected keyframe that is not
 * there (zeros in its two Sim3 rows; of a keyframe listed twice the last instance counts; without a usable current keyframe nothing
 * moves), a slot that is empty, a point whose normal is not written - and sets a bit in *d_status (nullable; zeroed first): 1 = offsets,
 * 2 = a keyframe index (conn_kf and its duplicates, obs_kf, ref_kf), 4 = a point index, 8 = conn_rank is not a permutation, 16 = a level,
 * 32 = Scw not finite or |q|^2 = 0 (the arithmetic still runs).  nd_written[p] is written for EVERY p here (0 where the point did not
 * move).  `d_workspace`: at least orbl_correct_loop_workspace(...) bytes, not shared with concurrent calls, reusable by the next.     */
int orbl_correct_loop_device(int nkf, double* d_kf_Tcw, double* d_kf_center, int nconn, const int32_t* d_conn_kf, const int32_t* d_conn_rank, const double* d_Scw,
                             int nslots, const int32_t* d_slot_off, const int32_t* d_slot_pt, int npts, double* d_X, const uint8_t* d_pt_bad,
                             const uint8_t* d_pt_done, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf, const int32_t* d_ref_kf,
                             const int32_t* d_ref_level, const float* d_scale_factors, int n_levels, double* d_corrected, double* d_non_corrected,
                             int32_t* d_pt_owner, double* d_normal, float* d_min_max, uint8_t* d_nd_written, int32_t* d_counts, uint32_t* d_status,
                             void* d_workspace, void* stream);
/* *bytes = the workspace orbl_correct_loop_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nconn, npts,
 * 4 * nkf, 8 * npts, 4 * nconn, 56 * nconn, 96 * nconn, 24 * nconn. */
int orbl_correct_loop_workspace(int nkf, int nconn, int npts, size_t* bytes);

/* ---- The write-back of the global bundle adjustment (LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:681-739): the walk of
 * the spanning tree from keyframe_origins_ that carries global_BA_Tcw_ to the keyframes created while the BA ran, and the move of every
 * map point to its BA position or through its reference keyframe's correction.
 *   kf_Tcw[nkf][12], kf_gba_Tcw[nkf][12] (global_BA_Tcw_), kf_in_gba[nkf] (n_BA_global_for_keyframe_ == nLoopKF): IN/OUT.
 *   kf_parent[nkf]: p iff the keyframe is in p->GetChilds(), else -1 (origins; bad keyframes, whose parent erased them).
 *   origin_kf[n_origin] = keyframe_origins_ (an origin's own parent entry is not read).  kf_center[nkf][3] (nullable, IN/OUT).
 *   X[npts][3] (IN/OUT), pt_bad (nullable), pt_in_gba / pt_gba_X[npts][3] (nullable as a pair), pt_ref_kf[npts].
 * A keyframe is REACHED when its parent chain ends in an origin.  A reached keyframe that is not in the BA gets
 * gba[c] = (Tcw[c] o Twc[parent]) o gba[parent] (the product and Twc of orbl_correct_loop; every right-hand operand at its value from
 * before any SetPose of this call) and is marked as in the BA.  Every reached keyframe k: kf_bef_Tcw[k] = Tcw[k] (global_BA_Bef_Tcw_; rows
 * of the others untouched), Tcw[k] = gba[k], the centre follows; kf_reached[nkf] is written for all.  A point that is not bad: in the BA:
 * X = pt_gba_X (pt_moved = 1); else with a reached reference keyframe: Xc = Rbef X + tbef, X = Rwc Xc + twc with the inverse of the NEW
 * pose (pt_moved = 2); else untouched (0).  counts[4] = {n_reached, n_propagated, n_points_moved, n_stale}.
 * ONE departure from the reference: a keyframe flagged as in the BA that the walk does not reach - the reference would read a stale
 * global_BA_Bef_Tcw_ for the points it is the reference of; here they stay put and are counted in n_stale.
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, NULLs, an origin,
 * parent (also k's own index) or reference keyframe out of range; a cycle among the parents leaves its keyframes unreached;
 * ORBHIP_ENODEV without a GPU.                                                                                                      */
int orbl_propagate_global_ba(int nkf, double* kf_Tcw, double* kf_gba_Tcw, uint8_t* kf_in_gba, const int32_t* kf_parent, int n_origin, const int32_t* origin_kf,
                             double* kf_center, int npts, double* X, const uint8_t* pt_bad, const uint8_t* pt_in_gba, const double* pt_gba_X,
                             const int32_t* pt_ref_kf, double* kf_bef_Tcw, uint8_t* kf_reached, uint8_t* pt_moved, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside.  Counts, NULL pointers and alignment are checked on
 * the host, the data on the device: an index out of range counts as absent (an origin that is not there, a keyframe without a parent, a
 * point that stays) and sets bit 1 of *d_status (nullable; zeroed first); 2 = a cycle in kf_parent (its keyframes are not reached);
 * 4 = n_stale > 0.  The tree is walked by one workgroup, one level per round, for any depth and any nkf.
 * `d_workspace`: at least orbl_propagate_global_ba_workspace(...) bytes, not shared with concurrent calls, reusable by the next.     */
int orbl_propagate_global_ba_device(int nkf, double* d_kf_Tcw, double* d_kf_gba_Tcw, uint8_t* d_kf_in_gba, const int32_t* d_kf_parent, int n_origin,
                                    const int32_t* d_origin_kf, double* d_kf_center, int npts, double* d_X, const uint8_t* d_pt_bad, const uint8_t* d_pt_in_gba,
                                    const double* d_pt_gba_X, const int32_t* d_pt_ref_kf, double* d_kf_bef_Tcw, uint8_t* d_kf_reached, uint8_t* d_pt_moved,
                                    int32_t* d_counts, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_propagate_global_ba_device needs (host arithmetic): nkf bytes rounded up to 256, at least 256. */
int orbl_propagate_global_ba_workspace(int nkf, int npts, size_t* bytes);

/* ---- CeresOptimizer::LocalBundleAdjustment on the map tables, first half (src/CeresOptimizer.cc:346-406 and the flattening :423-506):
 * the local keyframes, the local map points, the fixed keyframes, and one row per (local point, observing keyframe with a camera), as the
 * arguments of ba_local_bundle_adjustment.  Keyframes are 0..nkf-1, points 0..npts-1, nkf >= 1.
 *   cur_kf; nbr_kf[n_nbr] = GetVectorCovisibleKeyFrames() of it (bad ones, repeats and cur_kf itself allowed).
 *   kf_id[nkf]; kf_bad[nkf] (nullable); kf_rank[nkf] (nullable = index order): a permutation, the position under std::less<KeyFrame*>.
 *   kf_Tcw[nkf][12]; kf_K4[nkf][4] {fx, fy, cx, cy}, double.   kf_slot_off[nkf + 1] / kf_slot_pt[]: GetMapPointMatches() of EVERY
 *   keyframe, a point index or -1.   X[npts][3]; pt_bad (nullable); pt_rank[npts] (nullable = index order): std::less<MapPoint*>.
 *   obs_off[npts + 1] / obs_kf[] in each point's std::map order; obs_uv[nobs][2] (float, the undistorted keypoint); obs_level[nobs];
 *   inv_level_sigma2[n_levels].
 * Local keyframes: cur_kf and every nbr_kf that is not bad, each once.  A bad neighbour is still STAMPED local (:358) and so never becomes
 * fixed.  Local points: not bad, in a slot of a local keyframe.  Fixed keyframes: the observers of a local point that are neither stamped
 * nor bad.  Cameras: the local keyframes by ascending kf_id (ties: the current one, then nbr_kf order), then the fixed ones by ascending
 * kf_rank; cam_fixed[c] = fixed || kf_id == 0; cam_local[c]; poses7[c] = ba_matrix4d_to_pose7 of the pose; K4[c].  Points by ascending
 * pt_rank: lpt_pt[j], pts3[j].  Rows: per local point in that order its list in list order, without the observers that are bad or have no
 * camera: lobs_cam, lobs_pt, lobs_uv (double, the float widened), lobs_inv_sigma2 = inv_level_sigma2[obs_level], lobs_src = the index e in
 * the obs_* arrays.  A local point without rows stays in pts3.  kf_role[nkf] (0 none, 1 local, 2 fixed, 3 stamped local but bad) and
 * pt_local[npts] are written for every element.  counts[4] = {ncam, n_local_cam, npts_local, nobs_local}.
 * The output lists have the capacities cap_cam, cap_pts, cap_obs (an array may be NULL when its capacity is 0): when a list does not fit
 * the call returns ORBHIP_ECAP with only counts[] written.  Every place in a list comes from an ordered scan: the outputs are the same
 * bytes on every run.  Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts,
 * NULLs, cur_kf, offsets that do not ascend from 0, indices or levels out of range, ranks that are no permutations, n_levels outside
 * [1, 64]; ORBHIP_ENODEV without a GPU.                                                                                              */
int orbl_local_ba_assemble(int cur_kf, int n_nbr, const int32_t* nbr_kf, int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank, const double* kf_Tcw,
                           const double* kf_K4, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const double* X, const uint8_t* pt_bad,
                           const int32_t* pt_rank, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const int32_t* obs_level,
                           const float* inv_level_sigma2, int n_levels, int cap_cam, int cap_pts, int cap_obs, int32_t* counts, int32_t* cam_kf, double* K4,
                           double* poses7, uint8_t* cam_fixed, uint8_t* cam_local, int32_t* lpt_pt, double* pts3, int32_t* lobs_cam, int32_t* lobs_pt, double* lobs_uv,
                           float* lobs_inv_sigma2, int32_t* lobs_src, uint8_t* kf_role, uint8_t* pt_local);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nslots = kf_slot_off[nkf], nobs = obs_off[npts] given by
 * the caller; cur_kf is a host value and checked on the host).  Counts, NULL pointers and alignment (8 bytes for the 64-bit arrays and the
 * workspace, 4 for the 32-bit ones) are checked on the host; the data is bounds-checked on the device: an entry out of range counts as
 * ABSENT - a neighbour that is not there, an empty slot, a keyframe without slots, a point without a list, an observation that gives no
 * row - and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = a keyframe index, 4 = a point index, 8 = a rank is not a
 * permutation (of two holders of a place the higher index counts), 16 = a level; a list that does not fit is written up to its capacity,
 * counts[] holds the wanted sizes and 32 = cameras, 64 = points, 128 = rows is set.
 * `d_workspace`: at least orbl_local_ba_assemble_workspace(...) bytes, not shared with concurrent calls, reusable by the next.        */
int orbl_local_ba_assemble_device(int cur_kf, int n_nbr, const int32_t* d_nbr_kf, int nkf, const int32_t* d_kf_id, const uint8_t* d_kf_bad, const int32_t* d_kf_rank,
                                  const double* d_kf_Tcw, const double* d_kf_K4, int nslots, const int32_t* d_kf_slot_off, const int32_t* d_kf_slot_pt, int npts,
                                  const double* d_X, const uint8_t* d_pt_bad, const int32_t* d_pt_rank, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                  const float* d_obs_uv, const int32_t* d_obs_level, const float* d_inv_level_sigma2, int n_levels, int cap_cam, int cap_pts,
                                  int cap_obs, int32_t* d_counts, int32_t* d_cam_kf, double* d_K4, double* d_poses7, uint8_t* d_cam_fixed, uint8_t* d_cam_local,
                                  int32_t* d_lpt_pt, double* d_pts3, int32_t* d_lobs_cam, int32_t* d_lobs_pt, double* d_lobs_uv, float* d_lobs_inv_sigma2,
                                  int32_t* d_lobs_src, uint8_t* d_kf_role, uint8_t* d_pt_local, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_local_ba_assemble_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nkf, 4 * nkf,
 * 4 * npts, 4 * nkf, nkf, 8 * nkf, 8 * (ceil(nkf / 256) + 1), 8 * npts, 8 * (ceil(npts / 256) + 1), 16. */
int orbl_local_ba_assemble_workspace(int nkf, int npts, size_t* bytes);

/* ---- CeresOptimizer::LocalBundleAdjustment on the map tables, second half (src/CeresOptimizer.cc:573-598), in place on the tables.
 *   cam_kf[ncam], cam_local[ncam], lpt_pt[npts_local], lobs_src[nobs_local] as assembled; poses7[ncam][7], pts3[npts_local][3] and
 *   obs_erase[nobs_local] from ba_local_bundle_adjustment.
 *   IN/OUT: kf_Tcw[nkf][12], kf_center[nkf][3] (nullable unless normals are asked for), kf_slot_pt[], X[npts][3], pt_bad[npts],
 *   pt_nobs[npts] (= Observations()), pt_ref_kf[npts] (-1 = none: it is compared, and read only for a point that gets a normal).
 *   IN: kf_slot_off[nkf + 1], obs_off[npts + 1] / obs_kf[], obs_slot[nobs] (the observation's index in its keyframe), obs_level[nobs],
 *   kf_level0[nkf] (nullable = 0: the octave of keypoint 0), scale_factors[n_levels].
 * In this order:
 *  1. for every row i with obs_erase[i], in row order, e = lobs_src[i], k = obs_kf[e], p the point whose list holds e: nothing when e is no
 *     longer alive (GetIndexInKeyFrame == -1 / count() == 0 after a SetBadFlag); else slot obs_slot[e] of k becomes -1 whatever it held,
 *     the observation dies, pt_nobs[p]--; if pt_ref_kf[p] == k it becomes the observer of the first alive entry of the list (it stays when
 *     none is left: the ONE departure, the reference dereferences end() there); if pt_nobs[p] <= 2 the point turns bad and every alive
 *     observation of it dies with its slot set to -1 (pt_nobs is not reset).  Every observation listed at entry is alive.
 *  2. every camera with cam_local (kf_id == 0 included): Tcw = [R(q / |q|) | t] with the arithmetic of ba_pose7_to_matrix4d, the centre as
 *     orbl_correct_loop computes it.
 *  3. X[lpt_pt[j]] = pts3[j], bad points included.
 *  4. every local point that is not bad and has an alive observation: normal, min_max, nd_written = 1 as orbl_update_map_points computes
 *     them from the alive observations in list order, the NEW centres, pt_ref_kf[p] after step 1 and the level of the reference keyframe's
 *     alive observation - kf_level0[ref] when it has none (std::map::operator[], src/MapPoint.cc:366).  Rows of other points untouched.
 *   OUT: obs_erased[nobs] (every death of this call; every element written), nd_written[npts] (every element written), counts[4] =
 *   {n_erased (rows that found their observation alive), n_points_turned_bad, n_observations_dead, n_normals_written}.
 *   normal, min_max, nd_written and scale_factors are nullable AS A SET: then step 4 is left out (with npts = 0 the three arrays have no
 *   rows and may be NULL beside a given scale_factors).
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, NULLs, offsets,
 * indices, slots or levels out of range, a local camera's pose that is not finite or has |q| = 0; ORBHIP_ENODEV without a GPU.        */
int orbl_local_ba_apply(int ncam, const int32_t* cam_kf, const uint8_t* cam_local, const double* poses7, int npts_local, const int32_t* lpt_pt, const double* pts3,
                        int nobs_local, const int32_t* lobs_src, const uint8_t* obs_erase, int nkf, double* kf_Tcw, double* kf_center, const int32_t* kf_slot_off,
                        int32_t* kf_slot_pt, int npts, double* X, uint8_t* pt_bad, int32_t* pt_nobs, int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf,
                        const int32_t* obs_slot, const int32_t* obs_level, const int32_t* kf_level0, const float* scale_factors, int n_levels, uint8_t* obs_erased,
                        double* normal, float* min_max, uint8_t* nd_written, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside.  Counts, NULL pointers and alignment are checked on the
 * host, the data on the device: an entry out of range counts as absent (a row that erases nothing, a slot that is not written, a camera or
 * point that is not moved, a normal that is not written) and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = a keyframe
 * index, 4 = a point index, 16 = a level, 256 = lobs_src or obs_slot.
 * `d_workspace`: at least orbl_local_ba_apply_workspace(...) bytes, not shared with concurrent calls, reusable by the next.            */
int orbl_local_ba_apply_device(int ncam, const int32_t* d_cam_kf, const uint8_t* d_cam_local, const double* d_poses7, int npts_local, const int32_t* d_lpt_pt,
                               const double* d_pts3, int nobs_local, const int32_t* d_lobs_src, const uint8_t* d_obs_erase, int nkf, double* d_kf_Tcw,
                               double* d_kf_center, int nslots, const int32_t* d_kf_slot_off, int32_t* d_kf_slot_pt, int npts, double* d_X, uint8_t* d_pt_bad,
                               int32_t* d_pt_nobs, int32_t* d_pt_ref_kf, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf, const int32_t* d_obs_slot,
                               const int32_t* d_obs_level, const int32_t* d_kf_level0, const float* d_scale_factors, int n_levels, uint8_t* d_obs_erased,
                               double* d_normal, float* d_min_max, uint8_t* d_nd_written, int32_t* d_counts, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_local_ba_apply_device needs (host arithmetic): 4 * nobs bytes rounded up to 256, at least 256. */
int orbl_local_ba_apply_workspace(int nobs, size_t* bytes);

/* ---- CeresOptimizer::OptimizeEssentialGraph on the map tables, first half (src/CeresOptimizer.cc:769-905; LoopClosing.cc:573): the
 * vertices with the logarithms of their Sim(3)s and the edge list, as the arguments of ba_optimize_essential_graph.  Keyframes are
 * 0..nkf-1, nkf >= 1; map points do not enter.
 *   kf_id[nkf]; kf_bad[nkf] (nullable); kf_rank[nkf] (nullable = index order): a permutation, the position under std::less<KeyFrame*> -
 *   the order of Map::GetAllKeyFrames(), of loop_connections and of both std::set<KeyFrame*>.   kf_Tcw[nkf][12]; kf_parent[nkf]:
 *   GetParent() or -1.   child_off[nkf + 1] / child_kf[]: childrens_, read for hasChild only.   loop_off[nkf + 1] / loop_kf[]:
 *   GetLoopEdges(), rows in any order.   conn_off / conn_kf / conn_w: connected_keyframe_weights_, for GetWeight (0 when absent).
 *   ord_off[nkf + 1] / ord_kf / ord_w: ordered_connected_keyframes_ / ordered_weights_ (the layouts orbl_update_connections writes).
 *   nconn (>= 0), conn_group_kf[nconn], corrected[nconn][7], non_corrected[nconn][7]: the two KeyFrameAndSim3 maps as orbl_correct_loop
 *   returns them.   ntgt, tgt_kf[ntgt], link_off[ntgt + 1] / link_kf[]: loop_connections as orbl_update_connections returns it, rows in
 *   any order.   loop_keyframe, cur_keyframe: indices;   min_weight (100 at the call site, >= 1).
 * PRECONDITION: kf_id is distinct among the keyframes that are not bad (inserted_edges is keyed by id pairs; index pairs then say the same).
 *  1. Vertices: the keyframes that are not bad, numbered densely in ascending kf_rank: vtx_kf[v]; kf_vtx[k] (-1 = none, every element
 *     written); lie7[v] = log(corrected) for a keyframe of the group, else log(Sim3(RxSO3(1, Rcw), tcw)) with the matrix -> quaternion
 *     branches of ba_matrix4d_to_pose7; vtx_fixed[v] = (k == loop_keyframe).
 *  2. Loop-connection edges (:797-821): the targets in ascending kf_rank, each row in ascending kf_rank (a keyframe named twice counts
 *     once).  Entry (i, j) is skipped when (kf_id[i] != kf_id[cur] || kf_id[j] != kf_id[loop]) && GetWeight(i, j) < min_weight, and when an
 *     end has no vertex; else Sji = exp(lie[j]) * exp(lie[i])^-1 and the pair joins inserted_edges.
 *  3. Per keyframe i with a vertex, in ascending kf_rank, W(k) = non_corrected when k is in the group, else exp(lie[k]): the parent
 *     (:836-854); every loop edge l with kf_id[l] < kf_id[i], in ascending kf_rank (:857-876); of the prefix of the ordered list with
 *     ord_w >= min_weight - EMPTY when every weight of the list passes (KeyFrame::GetCovisiblesByWeight, src/KeyFrame.cc:218-235) - in list
 *     order the entries that are not the parent, not a child, not a loop edge, not bad, of smaller kf_id and not in inserted_edges
 *     (:879-905).  Every edge is Sji = W(j) * W(i)^-1 on (vertex j, vertex i); an edge to a keyframe without a vertex is not added.
 *   OUT: edge_j, edge_i (vertex numbers), edge_Sji[n_edges][7], edge_kind (0 loop connection, 1 parent, 2 loop edge, 3 covisibility);
 *   counts[4] = {n_vtx, n_edges, n_loop_connection_edges, n_dropped: entries every other rule admits of which an end has no vertex}.
 * Capacities cap_vtx, cap_edges (an array may be NULL when its capacity is 0): when a list does not fit the call returns ORBHIP_ECAP with
 * only counts[] written.  Every place comes from an ordered scan: the outputs are the same bytes on every run.  Host pointers,
 * synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, NULLs, loop_keyframe /
 * cur_keyframe, min_weight, offsets that do not ascend from 0, indices out of range, a rank that is no permutation, a keyframe twice in
 * conn_group_kf or tgt_kf, a corrected / non_corrected row that is not finite or has |q|^2 = 0, kf_id not distinct among the keyframes
 * that are not bad; ORBHIP_ENODEV without a GPU.                                                                                      */
int orbl_essential_graph_assemble(int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const int32_t* kf_rank, const double* kf_Tcw, const int32_t* kf_parent,
                                  const int32_t* child_off, const int32_t* child_kf, const int32_t* loop_off, const int32_t* loop_kf, const int32_t* conn_off,
                                  const int32_t* conn_kf, const int32_t* conn_w, const int32_t* ord_off, const int32_t* ord_kf, const int32_t* ord_w, int nconn,
                                  const int32_t* conn_group_kf, const double* corrected, const double* non_corrected, int ntgt, const int32_t* tgt_kf,
                                  const int32_t* link_off, const int32_t* link_kf, int loop_keyframe, int cur_keyframe, int min_weight, int cap_vtx, int cap_edges,
                                  int32_t* counts, int32_t* vtx_kf, int32_t* kf_vtx, double* lie7, uint8_t* vtx_fixed, int32_t* edge_j, int32_t* edge_i,
                                  double* edge_Sji, uint8_t* edge_kind);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (n_child = child_off[nkf], n_loop, n_connw, n_ord, n_link
 * likewise, given by the caller; loop_keyframe, cur_keyframe and min_weight are host values and checked on the host).  Counts, NULL
 * pointers and alignment (8 bytes for the 64-bit arrays and the workspace, 4 for the 32-bit ones) are checked on the host; the data is
 * bounds-checked on the device: an entry out of range counts as ABSENT - a parent, child, loop edge, connection, group member, target or
 * link that is not there, a row without entries - and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = a keyframe index
 * (or a keyframe twice in conn_group_kf / tgt_kf: its last instance counts), 8 = kf_rank is not a permutation (of two holders of a place
 * the higher index counts), 512 = a corrected / non_corrected row that is not finite or has |q|^2 = 0 (the keyframe counts as outside the
 * group); a list that does not fit is written up to its capacity and not beyond, d_counts holds the wanted sizes and 32 = vertices,
 * 64 = edges is set.
 * `d_workspace`: at least orbl_essential_graph_assemble_workspace(...) bytes, not shared with concurrent calls, reusable by the next. */
int orbl_essential_graph_assemble_device(int nkf, const int32_t* d_kf_id, const uint8_t* d_kf_bad, const int32_t* d_kf_rank, const double* d_kf_Tcw,
                                         const int32_t* d_kf_parent, int n_child, const int32_t* d_child_off, const int32_t* d_child_kf, int n_loop,
                                         const int32_t* d_loop_off, const int32_t* d_loop_kf, int n_connw, const int32_t* d_conn_off, const int32_t* d_conn_kf,
                                         const int32_t* d_conn_w, int n_ord, const int32_t* d_ord_off, const int32_t* d_ord_kf, const int32_t* d_ord_w, int nconn,
                                         const int32_t* d_conn_group_kf, const double* d_corrected, const double* d_non_corrected, int ntgt, const int32_t* d_tgt_kf,
                                         int n_link, const int32_t* d_link_off, const int32_t* d_link_kf, int loop_keyframe, int cur_keyframe, int min_weight,
                                         int cap_vtx, int cap_edges, int32_t* d_counts, int32_t* d_vtx_kf, int32_t* d_kf_vtx, double* d_lie7, uint8_t* d_vtx_fixed,
                                         int32_t* d_edge_j, int32_t* d_edge_i, double* d_edge_Sji, uint8_t* d_edge_kind, uint32_t* d_status, void* d_workspace,
                                         void* stream);
/* *bytes = the workspace orbl_essential_graph_assemble_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nkf,
 * 4 * nkf, 4 * nkf, 8 * nkf, 8 * (ceil(nkf / 256) + 1), 8 * nkf, 8 * (ceil(nkf / 256) + 1), 56 * nkf, 56 * nkf. */
int orbl_essential_graph_assemble_workspace(int nkf, size_t* bytes);

/* ---- CeresOptimizer::OptimizeEssentialGraph on the map tables, second half (src/CeresOptimizer.cc:916-956), in place on the tables.
 *   vtx_kf[n_vtx] as assembled, lie_orig[n_vtx][7] = the assembled lie7, lie_opt[n_vtx][7] from ba_optimize_essential_graph.
 *   IN/OUT: kf_Tcw[nkf][12], kf_center[nkf][3] (nullable unless normals are asked for), X[npts][3].
 *   IN: pt_bad (nullable), pt_done[npts] (nullable: corrected_by_keyframe_ == the current keyframe's id), pt_corr_ref[npts] (needed with
 *   pt_done: the keyframe index orbl_correct_loop returned as pt_owner), pt_ref_kf[npts] (-1 = none); for the normals, nullable AS A SET:
 *   obs_off[npts + 1] / obs_kf[], ref_level[npts], scale_factors[n_levels], normal, min_max, nd_written.
 *  1. every vertex keyframe: Tcw = [R | t / s] of exp(lie_opt) (the arithmetic of ba_essential_graph_correct), the centre as
 *     orbl_correct_loop computes it.
 *  2. every point that is not bad, r = pt_done ? pt_corr_ref : pt_ref_kf, r holding a vertex v: X <- exp(lie_opt[v])^-1 * (exp(lie_orig[v])
 *     * X), pt_moved = 1.  A point whose r is -1 or has no vertex stays and gets no normal (the reference would read an uninitialised
 *     block there).
 *  3. every moved point with observations: normal, min_max, nd_written = 1 as orbl_update_map_points computes them from the new position,
 *     pt_ref_kf, ref_level and the NEW centres (every SetPose precedes the point loop).  Rows of other points are untouched.
 *   OUT: pt_moved[npts] and nd_written[npts] (every element written), counts[2] = {n_poses_written, n_points_moved}.
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, NULLs, a keyframe
 * out of range or twice in vtx_kf, a tangent that is not finite, reference keyframes, observers or levels out of range, n_levels
 * outside [1, 64]; ORBHIP_ENODEV without a GPU.                                                                                      */
int orbl_essential_graph_apply(int n_vtx, const int32_t* vtx_kf, const double* lie_orig, const double* lie_opt, int nkf, double* kf_Tcw, double* kf_center, int npts, double* X,
                               const uint8_t* pt_bad, const uint8_t* pt_done, const int32_t* pt_corr_ref, const int32_t* pt_ref_kf, const int32_t* obs_off,
                               const int32_t* obs_kf, const int32_t* ref_level, const float* scale_factors, int n_levels, double* normal, float* min_max,
                               uint8_t* nd_written, uint8_t* pt_moved, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nobs = obs_off[npts]).  Counts, NULL pointers and
 * alignment are checked on the host, the data on the device: an entry out of range counts as absent (a vertex that writes no pose, a
 * point that stays, a normal that is not written) and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = a keyframe index
 * (or a keyframe twice in vtx_kf: its last vertex counts), 16 = a level, 512 = a tangent that is not finite.
 * `d_workspace`: at least orbl_essential_graph_apply_workspace(...) bytes, not shared with concurrent calls, reusable by the next.    */
int orbl_essential_graph_apply_device(int n_vtx, const int32_t* d_vtx_kf, const double* d_lie_orig, const double* d_lie_opt, int nkf, double* d_kf_Tcw, double* d_kf_center,
                                      int npts, double* d_X, const uint8_t* d_pt_bad, const uint8_t* d_pt_done, const int32_t* d_pt_corr_ref, const int32_t* d_pt_ref_kf,
                                      int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf, const int32_t* d_ref_level, const float* d_scale_factors, int n_levels,
                                      double* d_normal, float* d_min_max, uint8_t* d_nd_written, uint8_t* d_pt_moved, int32_t* d_counts, uint32_t* d_status,
                                      void* d_workspace, void* stream);
/* *bytes = the workspace orbl_essential_graph_apply_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nkf,
 * 56 * n_vtx, 56 * n_vtx; at least 256. */
int orbl_essential_graph_apply_workspace(int nkf, int n_vtx, size_t* bytes);

/* ---- CeresOptimizer::GlobalBundleAdjustemnt -> BundleAdjustment on the map tables, first half (src/CeresOptimizer.cc:59-176; called at
 * LoopClosing.cc:656 and Tracking.cc:502): the cameras, the points and one row per (point, observing keyframe with a camera), as the
 * arguments of ba_solve.  Keyframes are 0..nkf-1, points 0..npts-1 (both may be 0).
 *   ba_kf[n_ba_kf]: the `keyframes` argument (bad ones and repeats allowed); NULL = 0..nkf-1 (n_ba_kf is then nkf, or 0 for the empty list).
 *   ba_pt[n_ba_pt]: the `map_points` argument, DISTINCT (Map holds a std::set); NULL = 0..npts-1 (n_ba_pt is then npts, or 0).
 *   kf_id[nkf]; kf_bad[nkf] (nullable); kf_Tcw[nkf][12]; kf_K4[nkf][4] {fx, fy, cx, cy}, double.   X[npts][3]; pt_bad (nullable);
 *   obs_off[npts + 1] / obs_kf[] in each point's std::map order; obs_uv[nobs][2] (float, the undistorted keypoint); obs_level[nobs];
 *   inv_level_sigma2[n_levels]; is_robust.
 * Cameras: every ba_kf entry that is not bad, once (its FIRST list position counts), by ascending kf_id, ties by that first position (the
 * std::stable_sort of csrc/compat/orbslam_dropin.h); the ids need not be distinct, small or table indices.  cam_kf[c]; K4[c]; poses7[c] =
 * ba_matrix4d_to_pose7 of the pose; cam_fixed[c] = (kf_id == 0); kf_cam[nkf] = the camera or -1, every element written.
 * Points, in ba_pt order: a point that is not bad and has at least one row becomes problem point j: gpt_pt[j], pts3[j]; a point without
 * rows is LEFT OUT (:170-172; orbl_local_ba_assemble keeps such a point); pt_idx[npts] = j or -1, every element written.
 * Rows, per problem point in that order, its list in list order: one per observer that is not bad and has a camera - an observer outside
 * ba_kf gives no row.  The reference's gate id_ > max_keyframe_id (:142) is implied by "the observer has a camera": the maximum is taken
 * over the cameras, so no camera's id exceeds it; it is not tested a second time.  gobs_cam, gobs_pt, gobs_uv (double, the float widened),
 * gobs_weight = (double)inv_level_sigma2[obs_level], gobs_robust = is_robust ? 1 : 0, gobs_src = the index e in the obs_* arrays.
 * counts[3] = {ncam, npts_ba, nobs_ba}; all 0 when there is no camera (:67-70).
 * The output lists have the capacities cap_cam, cap_pts, cap_obs (an array may be NULL when its capacity is 0): when a list does not fit
 * the call returns ORBHIP_ECAP with only counts[] written.  Every place in a list comes from an ordered compaction: the outputs are the
 * same bytes on every run.  Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for
 * counts, NULLs, a NULL list whose count is neither 0 nor the table's, offsets that do not ascend from 0, indices or levels out of
 * range, a point twice in ba_pt, n_levels outside [1, 64]; ORBHIP_ENODEV without a GPU.                                               */
int orbl_global_ba_assemble(int n_ba_kf, const int32_t* ba_kf, int n_ba_pt, const int32_t* ba_pt, int nkf, const int32_t* kf_id, const uint8_t* kf_bad, const double* kf_Tcw,
                            const double* kf_K4, int npts, const double* X, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv,
                            const int32_t* obs_level, const float* inv_level_sigma2, int n_levels, int is_robust, int cap_cam, int cap_pts, int cap_obs, int32_t* counts,
                            int32_t* cam_kf, int32_t* kf_cam, double* K4, double* poses7, uint8_t* cam_fixed, int32_t* gpt_pt, int32_t* pt_idx, double* pts3,
                            int32_t* gobs_cam, int32_t* gobs_pt, double* gobs_uv, double* gobs_weight, uint8_t* gobs_robust, int32_t* gobs_src);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nobs = obs_off[npts] given by the caller).  Counts, NULL
 * pointers and alignment (8 bytes for the 64-bit arrays and the workspace, 4 for the 32-bit ones) are checked on the host; the data is
 * bounds-checked on the device exactly as in orbl_local_ba_assemble_device: an entry out of range counts as ABSENT - a list entry that is
 * not there, a point without a list, an observation that gives no row - and sets a bit in *d_status (nullable; zeroed first):
 * 1 = offsets, 2 = a keyframe index, 4 = a point index, 16 = a level; a list that does not fit is written up to its capacity, counts[]
 * holds the wanted sizes (kf_cam and pt_idx the wanted places) and 32 = cameras, 64 = points, 128 = rows is set.  1024 = a point twice in
 * ba_pt: its first position counts.
 * `d_workspace`: at least orbl_global_ba_assemble_workspace(...) bytes, not shared with concurrent calls, reusable by the next.       */
int orbl_global_ba_assemble_device(int n_ba_kf, const int32_t* d_ba_kf, int n_ba_pt, const int32_t* d_ba_pt, int nkf, const int32_t* d_kf_id, const uint8_t* d_kf_bad,
                                   const double* d_kf_Tcw, const double* d_kf_K4, int npts, const double* d_X, const uint8_t* d_pt_bad, int nobs,
                                   const int32_t* d_obs_off, const int32_t* d_obs_kf, const float* d_obs_uv, const int32_t* d_obs_level,
                                   const float* d_inv_level_sigma2, int n_levels, int is_robust, int cap_cam, int cap_pts, int cap_obs, int32_t* d_counts,
                                   int32_t* d_cam_kf, int32_t* d_kf_cam, double* d_K4, double* d_poses7, uint8_t* d_cam_fixed, int32_t* d_gpt_pt, int32_t* d_pt_idx,
                                   double* d_pts3, int32_t* d_gobs_cam, int32_t* d_gobs_pt, double* d_gobs_uv, double* d_gobs_weight, uint8_t* d_gobs_robust,
                                   int32_t* d_gobs_src, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_global_ba_assemble_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nkf, 4 * npts,
 * 8 * n_ba_kf, 4 * n_ba_kf, 16, 8 * n_ba_pt, 8 * (ceil(n_ba_pt / 256) + 1). */
int orbl_global_ba_assemble_workspace(int nkf, int npts, int n_ba_kf, int n_ba_pt, size_t* bytes);

/* ---- CeresOptimizer::BundleAdjustment on the map tables, second half (src/CeresOptimizer.cc:190-224), in place on the tables.
 *   cam_kf[ncam], gpt_pt[npts_ba] as assembled; poses7[ncam][7], pts3[npts_ba][3] from ba_solve.
 *   stage: 0 = n_loop_keyframe == 0 (Tracking::CreateInitialMapMonocular), 1 = n_loop_keyframe != 0 (RunGlobalBundleAdjustment).
 *   kf_bad[nkf], pt_bad[npts] (nullable) AT THE TIME OF THIS CALL: the reference tests isBad() again; a camera whose keyframe turned bad
 *   and a point that turned bad are skipped.
 * stage 0.  IN/OUT kf_Tcw[nkf][12], kf_center[nkf][3] (nullable unless normals are asked for), X[npts][3].
 *  1. every camera (kf_id == 0 included: constant in the solve, it still goes through the quaternion): Tcw = [R(q / |q|) | t] with the
 *     arithmetic of ba_pose7_to_matrix4d, the centre as orbl_correct_loop computes it.
 *  2. X[gpt_pt[j]] = pts3[j].
 *  3. every written point with observations: normal, min_max, nd_written = 1 as orbl_update_map_points computes them from the new
 *     position, pt_ref_kf, ref_level and the NEW centres (every SetPose precedes the point loop).  Rows of other points are untouched;
 *     nd_written[npts] is written for every element.  pt_ref_kf[npts] (-1 = none: no normal), obs_off[npts + 1] / obs_kf[],
 *     ref_level[npts], scale_factors[n_levels], normal[npts][3], min_max[npts][2] (float), nd_written are nullable AS A SET: then step 3
 *     is left out.  The stage-1 arrays are not read.
 * stage 1.  OUT kf_gba_Tcw[nkf][12] (that matrix, for the written keyframes), pt_gba_X[npts][3] (= pts3[j], for the written points),
 *  kf_in_gba[nkf] and pt_in_gba[npts]: EVERY element written, 1 where written and 0 elsewhere - the byte means
 *  n_BA_global_for_keyframe_ == nLoopKF, and this call is what sets that stamp.  These four are what orbl_propagate_global_ba reads.
 *  kf_Tcw, kf_center, X and the normal set are neither read nor written.
 * counts[3] = {n_poses_written, n_points_written, n_normals_written}.
 * Host pointers, synchronous, one packed upload and one download.  ORBHIP_EINVAL before any device work for counts, stage, NULLs, a
 * keyframe out of range or twice in cam_kf, a point out of range or twice in gpt_pt, a pose that is not finite or has |q| = 0, reference
 * keyframes, observers or levels out of range, n_levels outside [1, 64]; ORBHIP_ENODEV without a GPU.                                 */
int orbl_global_ba_apply(int ncam, const int32_t* cam_kf, const double* poses7, int npts_ba, const int32_t* gpt_pt, const double* pts3, int stage, int nkf,
                         const uint8_t* kf_bad, double* kf_Tcw, double* kf_center, int npts, double* X, const uint8_t* pt_bad, double* kf_gba_Tcw, uint8_t* kf_in_gba,
                         double* pt_gba_X, uint8_t* pt_in_gba, const int32_t* pt_ref_kf, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* ref_level,
                         const float* scale_factors, int n_levels, double* normal, float* min_max, uint8_t* nd_written, int32_t* counts);
/* The same with DEVICE pointers, enqueued on `stream`, no synchronisation inside (nobs = obs_off[npts]).  Counts, stage, NULL pointers and
 * alignment are checked on the host, the data on the device: an entry out of range counts as absent (a camera or a point that is not
 * written, a normal that is not written) and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = a keyframe index (or a
 * keyframe twice in cam_kf: its LAST camera counts), 4 = a point index (or a point twice in gpt_pt: its last place counts), 16 = a level,
 * 2048 = a pose that is not finite or has |q| = 0: that camera is not written.
 * `d_workspace`: at least orbl_global_ba_apply_workspace(...) bytes, not shared with concurrent calls, reusable by the next.          */
int orbl_global_ba_apply_device(int ncam, const int32_t* d_cam_kf, const double* d_poses7, int npts_ba, const int32_t* d_gpt_pt, const double* d_pts3, int stage, int nkf,
                                const uint8_t* d_kf_bad, double* d_kf_Tcw, double* d_kf_center, int npts, double* d_X, const uint8_t* d_pt_bad, double* d_kf_gba_Tcw,
                                uint8_t* d_kf_in_gba, double* d_pt_gba_X, uint8_t* d_pt_in_gba, const int32_t* d_pt_ref_kf, int nobs, const int32_t* d_obs_off,
                                const int32_t* d_obs_kf, const int32_t* d_ref_level, const float* d_scale_factors, int n_levels, double* d_normal, float* d_min_max,
                                uint8_t* d_nd_written, int32_t* d_counts, uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbl_global_ba_apply_device needs (host arithmetic), each section rounded up to 256 bytes: 4 * nkf, 4 * npts; at
 * least 256. */
int orbl_global_ba_apply_workspace(int nkf, int npts, size_t* bytes);

/* ---- Initializer::Initialize (src/Initializer.cc:54-889, monocular; called from src/Tracking.cc:432): the H / F RANSAC over
 * caller-given minimal sets, the model choice, ReconstructH / ReconstructF with CheckRT.  Frame 1 = the reference (initial) frame,
 * frame 2 = the current one.
 *   kps1[n1][2], kps2[n2][2]: undistorted keypoints {x, y}; matches12[n1]: frame-2 index or -1 (Tracking's init_matches_);
 *   K4 = {fx, fy, cx, cy} (Frame::K_); sigma (> 0) and iterations: the Initializer's constructor arguments (1.0, 200 at the call site);
 *   ransac_sets[iterations][8]: positions in the ascending list of matches (i1, matches12[i1]) - the sets :88-101 draw
 *     (DUtils::Random, seeded once per process: the library cannot see that sequence, so the sets are an input).
 * Outputs on success (report->reason == ORBT_INIT_OK): R21[9] (row-major), t21[3], P3D[n1][3] on the rows the winning motion
 * accepted (the other rows keep their values), triangulated[n1] on every row.  On rejection the four are left untouched.
 * report (always written): the chosen model (0 = H, 1 = F; -1 = none), the reason, both models' best scores and iterations
 * (-1 = no hypothesis scored above 0), RH, the inlier count of the chosen model's winner, the winning motion (-1 = none) and
 * nGood / parallax (degrees) per motion of the chosen model (4 used for F).
 * Reasons (the first rule of the reference that rejects, in its order):                                                         */
#define ORBT_INIT_OK 0
#define ORBT_INIT_BAD_INPUT 1      /* device entry only: counts, offsets, matches12 or set entries out of range, fewer than 8 matches */
#define ORBT_INIT_NO_MODEL 2       /* no hypothesis of the chosen model scored above 0 (the reference reads an uninitialised matrix) */
#define ORBT_INIT_H_DEGENERATE 3   /* ReconstructH: d1 / d2 < 1.00001 or d2 / d3 < 1.00001 (:573) */
#define ORBT_INIT_H_AMBIGUOUS 4    /* ReconstructH: secondBestGood >= 0.75 bestGood (:683) */
#define ORBT_INIT_H_PARALLAX 5     /* ReconstructH: bestParallax < minParallax = 1 */
#define ORBT_INIT_H_FEW 6          /* ReconstructH: bestGood <= 50 or bestGood <= 0.9 N */
#define ORBT_INIT_F_FEW 7          /* ReconstructF: maxGood < max(int(0.9 N), 50) (:496) */
#define ORBT_INIT_F_AMBIGUOUS 8    /* ReconstructF: more than one motion with nGood > 0.7 maxGood */
#define ORBT_INIT_F_PARALLAX 9     /* ReconstructF: the first motion with nGood == maxGood has parallax <= 1 (no fall-through, :501-537) */
#define ORBT_INIT_MAX_N 32768      /* keypoints per frame */
#define ORBT_INIT_MAX_ITERATIONS 4096
#define ORBT_INIT_MAX_PAIRS 65535
typedef struct orbt_init_report {
  int32_t model, reason;
  float score_h, score_f, rh;
  int32_t best_h, best_f;
  int32_t n_matches, n_inliers;
  int32_t motion;
  int32_t n_good[8];
  float parallax[8];
} orbt_init_report;
/* Optional per-call trace (host entry only; every member nullable): the per-iteration H21, H12, F21 [iterations][9] exactly as the
 * scoring consumed them, the per-iteration scores [iterations], the chosen model's motions R [8][9] / t [8][3] (zero where the model
 * has fewer or none were made) and the H and F winners' inlier masks [n_matches] (0 where the model has no winner).             */
typedef struct orbt_init_trace {
  double* H21; double* H12; double* F21;
  float* score_h; float* score_f;
  double* motion_R; double* motion_t;
  uint8_t* inliers_h; uint8_t* inliers_f;
} orbt_init_trace;
/* Host pointers, synchronous.  ORBHIP_EINVAL before any device work for n1 / n2 outside [0, 32768], iterations outside [1, 4096],
 * sigma <= 0 (or not finite), fewer than 8 matches, matches12 entries outside [-1, n2), set entries outside [0, n_matches) and NULL
 * required pointers.  It is orbt_initialize_batch_device with one pair.                                                           */
int orbt_initialize(const float* kps1, int n1, const float* kps2, int n2, const int32_t* matches12, const float* K4, float sigma, int iterations,
                    const int32_t* ransac_sets, double* R21, double* t21, double* P3D, uint8_t* triangulated, orbt_init_report* report,
                    const orbt_init_trace* trace);
/* The same for npairs pairs with DEVICE pointers, enqueued on `stream`: pair p's keypoints are rows off1[p] .. off1[p+1] of
 * kps1 [n1_total][2] (off2 / kps2 likewise; CSR, device arrays), its matches12, P3D and triangulated rows share kps1's offsets,
 * K4[p][4], ransac_sets[p][iterations][8], R21[p][9], t21[p][3], report[p].  One sigma and iterations for all pairs.
 * Counts, sigma and NULL pointers are checked on the host; the data is not read there, so a pair whose offsets, matches12 or set
 * entries are out of range, or that has fewer than 8 matches, fails alone with ORBT_INIT_BAD_INPUT.  `workspace`: device memory of
 * orbt_initialize_workspace() bytes, not shared with concurrent calls.  No allocation, no host synchronisation.                 */
int orbt_initialize_batch_device(int npairs, const float* d_kps1, const int32_t* d_off1, int n1_total, const float* d_kps2, const int32_t* d_off2,
                                 int n2_total, const int32_t* d_matches12, const float* d_K4, float sigma, int iterations, const int32_t* d_ransac_sets,
                                 double* d_R21, double* d_t21, double* d_P3D, uint8_t* d_triangulated, orbt_init_report* d_report, void* d_workspace,
                                 void* stream);
/* *bytes = the workspace orbt_initialize_batch_device needs (host arithmetic); npairs in [1, 65535], n*_total <= 32768 npairs. */
int orbt_initialize_workspace(int npairs, int n1_total, int n2_total, int iterations, size_t* bytes);

/* ---- PnPsolver (src/PnPsolver.cc; called from Tracking::Relocalization, src/Tracking.cc:1003-1060): EPnP inside RANSAC, one
 * `iterate` call per candidate and library call, for a batch of candidates.
 *   p3d[n][3]: the matched map points' world positions narrowed to float (mvP3Dw, :93-94); p2d[n][2]: the undistorted keypoints
 *   (mvP2D); max_err[n] = level_sigma2[octave] * th2 (mvMaxError, :155-157); K4 = {fx, fy, cx, cy}.  The caller compacts the non-NULL,
 *   non-bad matches (:79-102) and scatters the returned mask through mvKeyPointIndices (:232-237).
 *   min_inliers: the ADJUSTED mRansacMinInliers of orbt_pnp_ransac_params (>= 4).
 *   sets[n_sets][4]: the minimal sets, indices into the n points, distinct inside a set - what :192-203 draws from DUtils::Random
 *     (process-global, drawn lazily between candidates: the library cannot see that sequence, so the sets are an input).  One
 *     `iterate(nIterations, ...)` call of the reference runs while `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`
 *     (:183), so the caller supplies n_sets = max(mRansacMaxIts - mnIterations, nIterations) sets and advances mnIterations by
 *     result->consumed; a call always ends with a refined pose or with every set used.
 *   best_count / best_mask[n] / best_Tcw[16] (row-major 4 x 4): mnBestInliers, mvbBestInliers, mBestTcw - in/out, zero / zeros /
 *     anything before the first call.  best_count must equal the number of non-zero mask bytes.
 * Per iteration (:183-242): compute_pose on the set (EPnP, double), CheckInliers (:313-345, the reference's float / double mix); with
 * count >= min_inliers a count STRICTLY above best_count becomes the state, then Refine (:263-310) refits on the BEST mask and returns
 * its pose when the refit has STRICTLY more than min_inliers inliers.
 * result (always written except Tcw on BAD_INPUT): status, consumed = the sets the reference would have used before returning,
 * Tcw (row-major; identity where the reference returns identity), n_inliers, n_refits = Refine calls made (one per distinct best mask:
 * a mask that failed is not refitted again, the outcome is the same).  inliers[n]: the refined mask (REFINED), the best mask
 * (EXHAUSTED_BEST) or zeros.  The state is as of iteration `consumed`; sets after it leave no trace in any output.
 * Parity: EPnP takes rows 8-11 of cvSVD's Ut of the 12 x 12 MtM; with 4 points MtM has a null space of dimension >= 4 and those rows
 * are an arbitrary basis of it, so a hypothesis' pose depends on the eigen-solver and equality with an OpenCV build is not attainable
 * hypothesis by hypothesis ("PnP RANSAC").  tests/nppnp.py restates this implementation's operation order. */
#define ORBT_PNP_REFINED 0         /* Refine succeeded at iteration consumed - 1: Tcw = mRefinedTcw, inliers = mvbRefinedInliers */
#define ORBT_PNP_EXHAUSTED_BEST 1  /* every set used, best_count >= min_inliers: Tcw = mBestTcw, inliers = mvbBestInliers, bNoMore */
#define ORBT_PNP_EXHAUSTED_NONE 2  /* every set used, no hypothesis reached min_inliers: identity, bNoMore */
#define ORBT_PNP_TOO_FEW 3         /* n < min_inliers (:174-178): identity, bNoMore, consumed = 0, the state untouched */
#define ORBT_PNP_BAD_INPUT 4       /* device entry only: offsets, n_sets, min_inliers < 4, a set entry out of range or repeated, a state that does not match */
#define ORBT_PNP_MAX_N 32768       /* points per candidate */
#define ORBT_PNP_MAX_ITERATIONS 4096
#define ORBT_PNP_MAX_CANDIDATES 65535
typedef struct orbt_pnp_params {
  int32_t n, min_inliers, max_iterations;      /* N, the adjusted mRansacMinInliers and mRansacMaxIts */
  float epsilon;                               /* the adjusted mRansacEpsilon */
} orbt_pnp_params;
typedef struct orbt_pnp_result {
  int32_t status, consumed, n_inliers, n_refits;
  double Tcw[16];
} orbt_pnp_result;
/* Optional per-call trace (host entry only; every member nullable), rows [n_sets]: per consumed iteration the hypothesis' R [9] and
 * t [3], the approximation compute_pose chose (1..3, :523-525), its mean reprojection error and the inlier count (zeros beyond
 * `consumed`); per Refine call k < n_refits the iteration that made it, its R, t and count (iteration -1 beyond n_refits).          */
typedef struct orbt_pnp_trace {
  double* R; double* t; int32_t* approx; double* rep_error; int32_t* count;
  int32_t* refit_iteration; double* refit_R; double* refit_t; int32_t* refit_count;
} orbt_pnp_trace;
/* SetRansacParameters' arithmetic (:122-153) on the host: out->min_inliers = max(int(n * epsilon), min_inliers, min_set),
 * out->epsilon = max(epsilon, min_inliers / n), out->max_iterations = max(1, min(ceil(log(1 - p) / log(1 - epsilon^3)),
 * max_iterations)), 1 when min_inliers == n or when the quotient is not a number (n < min_inliers).  ORBHIP_EINVAL for min_set != 4
 * (the reference uses no other value and EPnP on fewer points is undefined), n outside [0, 32768], probability outside (0, 1),
 * epsilon outside (0, 1], min_inliers < 0, max_iterations < 1.                                                                   */
int orbt_pnp_ransac_params(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon, orbt_pnp_params* out);
/* One candidate, host pointers, synchronous.  ORBHIP_EINVAL before any device work for n outside [0, 32768], n_sets outside
 * [0, 4096], min_inliers < 4, NULL required pointers and, when n >= min_inliers, set entries outside [0, n), an index repeated inside
 * a set, or a best_count that is not the number of non-zero best_mask bytes.  It is orbt_pnp_iterate_batch_device with one candidate. */
int orbt_pnp_iterate(const float* p3d, const float* p2d, const float* max_err, int n, const float* K4, int min_inliers, const int32_t* sets, int n_sets,
                     int32_t* best_count, uint8_t* best_mask, double* best_Tcw, orbt_pnp_result* result, uint8_t* inliers, const orbt_pnp_trace* trace);
/* The same for n_candidates candidates with DEVICE pointers, enqueued on `stream`: candidate c's points are rows off[c] .. off[c+1]
 * of p3d / p2d / max_err / best_mask / inliers (CSR, device array of n_candidates + 1), K4[c][4], min_inliers[c], n_sets[c] <=
 * iterations, sets[c][iterations][4], best_count[c], best_Tcw[c][16], result[c].  Counts and NULL pointers are checked on the host;
 * the data is not read there, so a candidate with bad offsets, n_sets, min_inliers, set entries or state fails alone with
 * ORBT_PNP_BAD_INPUT (its result gets the status, everything else of it stays as it was).  `workspace`: device memory of
 * orbt_pnp_iterate_workspace() bytes, not shared with concurrent calls.  No allocation, no host synchronisation.                 */
int orbt_pnp_iterate_batch_device(int n_candidates, const float* d_p3d, const float* d_p2d, const float* d_max_err, const int32_t* d_off, int n_total,
                                  const float* d_K4, const int32_t* d_min_inliers, const int32_t* d_n_sets, int iterations, const int32_t* d_sets,
                                  int32_t* d_best_count, uint8_t* d_best_mask, double* d_best_Tcw, orbt_pnp_result* d_result, uint8_t* d_inliers,
                                  void* d_workspace, void* stream);
/* *bytes = the workspace orbt_pnp_iterate_batch_device needs (host arithmetic); n_candidates in [1, 65535], n_total <= 32768
 * n_candidates, iterations in [1, 4096].                                                                                         */
int orbt_pnp_iterate_workspace(int n_candidates, int n_total, int iterations, size_t* bytes);

/* ---- Sim3Solver (src/Sim3Solver.cc; called from LoopClosing::ComputeSim3, src/LoopClosing.cc:269-317): Horn's closed-form Sim(3)
 * from three correspondences inside RANSAC, one `iterate` call per candidate and library call, for a batch of loop candidates.
 *   X1c[n][3], X2c[n][3] double: the matched map points in each keyframe's camera frame, Rcw * Xw + tcw (X3Dsc1_, X3Dsc2_, :100-104).
 *   max_err1[n], max_err2[n] float: max_errors_1_ / _2_ - the reference keeps them in std::vector<size_t>, so they hold
 *     9.210 * level_sigma2[octave] TRUNCATED to an integer (:93-94); the caller passes the truncated values.
 *   K1[4], K2[4] = {fx, fy, cx, cy} of the two keyframes; fix_scale = is_fixed_scale_ (scale = 1.0f).
 *   The caller compacts the matches by the constructor's skip rules (:73-85) and scatters the returned mask through
 *   matched_indices_1_ (:200-203).
 *   min_inliers: ransac_min_inliers_ (>= 3).
 *   sets[n_sets][3]: the minimal sets, indices into the n correspondences, distinct inside a set - what :169-182 draws from
 *     DUtils::Random (process-global, drawn lazily between candidates: the library cannot see that sequence, so the sets are an input).
 *     One `iterate(n_iterations, ...)` call of the reference runs while `n_iterations_ < ransac_max_iterations_ &&
 *     n_current_iterations < n_iterations` (:164-165, an AND), so the caller supplies n_sets = min(ransac_max_iterations_ -
 *     n_iterations_, n_iterations) sets, advances n_iterations_ by result->consumed, and sets is_no_more when the call ends without
 *     success and n_iterations_ has reached ransac_max_iterations_ (:209).
 *   best_count / best_mask[n] / best_R[9] (row-major) / best_t[3] / best_scale: n_best_inliers_, is_best_inliers_, best_rotation_,
 *     best_translation_, best_scale_ - in/out, zero / zeros / anything before the first call.  best_count must equal the number of
 *     non-zero mask bytes.
 * Per set (:184-206): ComputeSim3 (double; the scale narrowed to float as scale_12_i_ is), CheckInliers (:365-385) with the reference's
 * float / double mix; a count >= best_count becomes the state (ties go to the LATER set), and the call returns when such a count is
 * STRICTLY above min_inliers.  A degenerate triple gives a non-finite hypothesis whose count is 0; like the reference it can enter the
 * state while best_count is 0.
 * result (always written except the pose on BAD_INPUT): status, consumed = the sets the reference would have used before returning,
 * n_inliers, T12 (row-major [s R | t]; identity where the reference returns identity), R, t, scale = the state after the call (what
 * GetEstimatedRotation / Translation / Scale return).  inliers[n]: the best mask (FOUND) or zeros.  Sets after `consumed` leave no
 * trace in any output.
 * The eigenvector of Horn's 4 x 4 N comes from a two-sided Jacobi (the reference: Eigen::EigenSolver); the rotation is unique where
 * the two largest eigenvalues are apart, and tests/npsim3solver.py restates this implementation's operation order (DESIGN.md section 2,
 * "Sim3 RANSAC"). */
#define ORBT_SIM3_FOUND 0          /* set consumed - 1 reached more than min_inliers inliers: T12 = best_T12_, inliers = is_best_inliers_ */
#define ORBT_SIM3_NOT_FOUND 1      /* every given set used without success: identity, no inliers; the state holds the best so far */
#define ORBT_SIM3_TOO_FEW 2        /* n < min_inliers (:153-156): identity, is_no_more, consumed = 0, the state untouched */
#define ORBT_SIM3_BAD_INPUT 3      /* device entry only: offsets, n_sets, min_inliers < 3, a set entry out of range or repeated, a state that does not match */
#define ORBT_SIM3_MAX_N 32768      /* correspondences per candidate */
#define ORBT_SIM3_MAX_ITERATIONS 4096
#define ORBT_SIM3_MAX_CANDIDATES 65535
typedef struct orbt_sim3_params {
  int32_t n, min_inliers, max_iterations, reserved;   /* N_, ransac_min_inliers_ and the adjusted ransac_max_iterations_ */
} orbt_sim3_params;
typedef struct orbt_sim3_result {
  int32_t status, consumed, n_inliers;
  float scale;
  double T12[16], R[9], t[3];
} orbt_sim3_result;
/* Optional per-call trace (host entry only; every member nullable), rows [n_sets]: per consumed set the hypothesis' R [9], t [3],
 * scale (the float, widened), the inlier count and relgap = (l3 - l2) / l3 of the two largest eigenvalues of N (zeros beyond
 * `consumed`). */
typedef struct orbt_sim3_trace {
  double* R; double* t; double* scale; int32_t* count; double* relgap;
} orbt_sim3_trace;
/* SetRansacParameters' arithmetic (:131-142) on the host: epsilon = (float)min_inliers / n, out->max_iterations = max(1,
 * min(ceil(log(1 - p) / log(1 - epsilon^3)), max_iterations)), 1 when min_inliers == n.  For n < min_inliers the reference's quotient
 * is not a number (log of a negative); out->max_iterations = 1 then - iterate never uses the value in that case.  ORBHIP_EINVAL for n
 * outside [0, 32768], probability outside (0, 1), min_inliers < 0, max_iterations < 1. */
int orbt_sim3_ransac_params(int n, double probability, int min_inliers, int max_iterations, orbt_sim3_params* out);
/* One candidate, host pointers, synchronous.  ORBHIP_EINVAL before any device work for n outside [0, 32768], n_sets outside
 * [0, 4096], min_inliers < 3, NULL required pointers and, when n >= min_inliers, set entries outside [0, n), an index repeated inside
 * a set, or a best_count that is not the number of non-zero best_mask bytes.  It is orbt_sim3_iterate_batch_device with one candidate. */
int orbt_sim3_iterate(const double* X1c, const double* X2c, const float* max_err1, const float* max_err2, int n, const float* K1, const float* K2,
                      int fix_scale, int min_inliers, const int32_t* sets, int n_sets, int32_t* best_count, uint8_t* best_mask, double* best_R,
                      double* best_t, float* best_scale, orbt_sim3_result* result, uint8_t* inliers, const orbt_sim3_trace* trace);
/* The same for n_candidates candidates with DEVICE pointers, enqueued on `stream`: candidate c's correspondences are rows off[c] ..
 * off[c+1] of X1c / X2c / max_err1 / max_err2 / best_mask / inliers (CSR, device array of n_candidates + 1), K1[c][4], K2[c][4],
 * fix_scale[c], min_inliers[c], n_sets[c] <= iterations, sets[c][iterations][3], best_count[c], best_R[c][9], best_t[c][3],
 * best_scale[c], result[c].  X1c / X2c with `off` are the P3D1c / P3D2c / offsets arguments of ba_optimize_sim3_batch_device, and
 * best_R / best_t / best_scale / inliers stay on the device per candidate, so a caller goes on to SearchBySim3 and OptimizeSim3
 * without a round trip.  Counts and NULL pointers are checked on the host; the data is not read there, so a candidate with bad
 * offsets, n_sets, min_inliers, set entries or state fails alone with ORBT_SIM3_BAD_INPUT (its result gets the status, everything else
 * of it stays as it was).  `workspace`: device memory of orbt_sim3_iterate_workspace() bytes, not shared with concurrent calls.  No
 * allocation, no host synchronisation. */
int orbt_sim3_iterate_batch_device(int n_candidates, const double* d_X1c, const double* d_X2c, const float* d_max_err1, const float* d_max_err2,
                                   const int32_t* d_off, int n_total, const float* d_K1, const float* d_K2, const int32_t* d_fix_scale,
                                   const int32_t* d_min_inliers, const int32_t* d_n_sets, int iterations, const int32_t* d_sets, int32_t* d_best_count,
                                   uint8_t* d_best_mask, double* d_best_R, double* d_best_t, float* d_best_scale, orbt_sim3_result* d_result,
                                   uint8_t* d_inliers, void* d_workspace, void* stream);
/* *bytes = the workspace orbt_sim3_iterate_batch_device needs (host arithmetic); n_candidates in [1, 65535], n_total <= 32768
 * n_candidates, iterations in [1, 4096]. */
int orbt_sim3_iterate_workspace(int n_candidates, int n_total, int iterations, size_t* bytes);

/* ---- the per-frame Tracking step with the motion model, device-resident (src/Tracking.cc:616-646): Frame construction
 * (ORBextractor::operator(), UndistortKeyPoints with the coefficients orbt_set_distortion attached to ctx - none by default, as for
 * the KITTI configurations: the undistorted keypoints are then the raw ones -, AssignFeaturesToGrid), ORBmatcher::SearchByProjection(current_frame_, last_frame_, th) (src/ORBmatcher.cc:1161-1271,
 * monocular) and CeresOptimizer::PoseOptimization (src/CeresOptimizer.cc:275-342) in ONE call: the image and one packed block
 * go up, the kernels of all three stages run back to back on one stream (the greedy, order-dependent pass of the search as a
 * parallel fixpoint on the device, csrc/orb_track.hip), one block comes down.
 *   in   img: CV_8UC1 w x h; K4 = {fx, fy, cx, cy}; bounds = {min_x, max_x, min_y, max_y} from orbt_image_bounds with the SAME
 *        coefficients as orbt_set_distortion got (the grid and the projection test use them); Tcw_pred = current_frame_.Tcw_
 *        after SetPose(velocity_ * last_frame_.Tcw_), row-major 3x4 (or the first 12 of a 4x4); per last-frame feature i
 *        (n_last <= 4096): last_Xw = map point position, last_desc = its descriptor (MapPoint::GetDescriptor), last_octave =
 *        LastFrame.keypoints_[i].octave, last_angle = LastFrame.undistort_keypoints_[i].angle, last_valid = 0 (no map point,
 *        or is_outliers_[i]), 1 (map point with Observations() > 0) or 3 (without: it is matched but does not close the
 *        feature for later points, :1220-1221); th = 15 (the caller repeats the call with 2 * th when nmatches < 20,
 *        src/Tracking.cc:635-641); check_ori = mbCheckOrientation.
 *   out  kps / desc [cap >= orbx_max_keypoints(ctx)]: the frame's RAW keypoints (keypoints_) and descriptors - the undistorted
 *        ones (undistort_keypoints_[i].pt) are orbt_last_undistorted_keypoints' -; match[n_last]: index of the
 *        current feature matched to last-frame feature i, -1 none, -2 - index removed by the rotation check; owner[n_kp]:
 *        which last-frame feature's map point CurrentFrame.map_points_[f] holds, or -1; outlier[n_kp] = is_outliers_ after
 *        PoseOptimization; res: counts, the optimised pose [tx, ty, tz, qx, qy, qz, qw] (the predicted one when fewer than
 *        3 correspondences, as the reference leaves the pose alone then).                                                  */
typedef struct orbt_result {
  int32_t n_keypoints, nmatches, n_correspondences, n_inliers, greedy_rounds, reserved;
  double pose7[7];
} orbt_result;
int orbt_track_with_motion_model(orbx_ctx* ctx, const uint8_t* img, int w, int h, int stride, const float* K4, const float* bounds,
                                 const double* Tcw_pred, const double* last_Xw, const uint8_t* last_desc, const int32_t* last_octave,
                                 const float* last_angle, const uint8_t* last_valid, int n_last, float th, int check_ori,
                                 orbx_keypoint* kps_out, uint8_t* desc_out, int cap, int32_t* match_out, int32_t* owner_out,
                                 uint8_t* outlier_out, orbt_result* res);

/* ---- the second stage of Tracking on the same frame, device-resident (src/Tracking.cc:673-750 TrackLocalMap): SearchLocalPoints
 * (:793-842) = Frame::isInFrustum(pMP, 0.5) (src/Frame.cc:191-241, MapPoint::PredictScale src/MapPoint.cc:406-420) over the local
 * map points, ORBmatcher::SearchByProjection(Frame&, vpMapPoints, th) (src/ORBmatcher.cc:42-119: window radius by viewing cosine,
 * levels [nPredictedLevel - 1, nPredictedLevel], best / second best + level rule, nnratio, the :83-84 claim rule), then
 * CeresOptimizer::PoseOptimization over EVERY slot that holds a point - in ONE call on the frame (keypoints, descriptors, grid)
 * that orbt_track_with_motion_model left on the device: the same host thread must have called it for this frame.
 *   in   Tcw = current_frame_.Tcw_ (row-major 3x4: the pose the first stage optimised); log_scale_factor = Frame::log_scale_factor_;
 *        per local map point (n_mp <= 16384, vector order of local_map_points_): position, GetNormal(), min_distance_ /
 *        max_distance_ (the 0.8 / 1.2 invariance factors are applied inside), GetDescriptor(), mp_state = 0 skip (isBad(), or
 *        last_seen_frame_id_ == current_frame_.id_: it already sits in the frame, :816-817), 1 candidate with Observations() > 0,
 *        3 candidate without (it is matched but does not close the feature, :83-84); per keypoint of the frame
 *        (n_kp = the resident frame's count): slot_state = 0 empty, 1 holds a point with Observations() > 0 (closed), 3 holds one
 *        without; slot_Xw = that point's position (read where slot_state != 0); th = 1 (5 right after a relocalisation,
 *        :834-838), nnratio = 0.8.
 *   out  mp_in_view[n_mp] = isInFrustum result (the caller's IncreaseVisible, :822-825); mp_match[n_mp] = feature the point was
 *        written to or -1; slot_owner[n_kp] = index of the local map point the slot holds NOW if this call wrote it (the last
 *        writer, :110), else -1 (unchanged); outlier[n_kp] = is_outliers_ after PoseOptimization; res: nmatches, correspondences,
 *        inliers, pose (the input pose with fewer than 3 correspondences), reserved = points in view.                          */
int orbt_track_local_map(orbx_ctx* ctx, const float* K4, const float* bounds, const double* Tcw, float log_scale_factor,
                         const double* mp_Xw, const double* mp_normal, const float* mp_min_dist, const float* mp_max_dist,
                         const uint8_t* mp_desc, const uint8_t* mp_state, int n_mp, const double* slot_Xw, const uint8_t* slot_state,
                         int n_kp, float th, float nnratio, uint8_t* mp_in_view, int32_t* mp_match, int32_t* slot_owner,
                         uint8_t* outlier, orbt_result* res);
/* The same with the map-point and slot arrays as DEVICE pointers: the packed mp_* / slot_* arrays orbt_update_local_map_device wrote on
 * `stream` (the call's own stream waits for the work enqueued on `stream` so far; NULL = the default stream).  n_mp is given by the
 * caller: at least the number of local map points and at most 16384 - the rows from the count up to cap_pt carry mp_state = 0, so
 * n_mp = cap_pt needs no knowledge of the count; such rows come back as "not in view, -1".  The arrays d_mp_Xw, d_mp_normal and
 * d_slot_Xw are 8-byte, d_mp_min_dist and d_mp_max_dist 4-byte, d_mp_desc 16-byte aligned.  Outputs are host arrays, the call is synchronous, and it
 * runs the same kernels on the same bytes as orbt_track_local_map: the results are identical.                                     */
int orbt_track_local_map_device(orbx_ctx* ctx, const float* K4, const float* bounds, const double* Tcw, float log_scale_factor,
                                const double* d_mp_Xw, const double* d_mp_normal, const float* d_mp_min_dist, const float* d_mp_max_dist,
                                const uint8_t* d_mp_desc, const uint8_t* d_mp_state, int n_mp, const double* d_slot_Xw,
                                const uint8_t* d_slot_state, int n_kp, float th, float nnratio, void* stream, uint8_t* mp_in_view,
                                int32_t* mp_match, int32_t* slot_owner, uint8_t* outlier, orbt_result* res);

/* ---- Tracking::UpdateLocalMap (src/Tracking.cc:838-977) = UpdateLocalKeyFrames (:874-977) + UpdateLocalPoints (:847-872), and what
 * SearchLocalPoints (:793-826) fixes from that state, so that the result IS orbt_track_local_map's input.  All ids are int32.
 *   points 0..npts-1: pt_bad (isBad()), pt_nobs (Observations()), the observers as CSR obs_off[npts + 1] into obs_kf[] (any order
 *     within a point), the records pt_Xw[3] / pt_normal[3] (double), pt_min_dist / pt_max_dist (float), pt_desc[32].
 *   keyframes 0..nkf-1: kf_bad; kf_rank[nkf], a permutation: the position of the keyframe in the caller's std::map<KeyFrame*, ...>
 *     order (the reference iterates keyframeCounter in pointer order, :906; NULL = index order); kf_parent (-1 = none); the best
 *     covisibles as CSR cov_off / cov_kf, at most 10 per keyframe in GetBestCovisibilityKeyFrames(10) order; the children as CSR
 *     child_off / child_kf in the caller's std::set order; the slot table as CSR kf_slot_off / kf_slot_pt (point id or -1).
 *   frame: frame_pt[n_kp] (point id or -1); seen_pt[n_seen]: the points whose last_seen_frame_id_ already equals the current frame id
 *     without sitting in a slot (the outliers TrackWithMotionModel discarded, :655-659); prev_local_kf[n_prev <= nkf]: local_keyframes_
 *     of the frame before.
 *   PRECONDITION: no keyframe or point carries track_reference_for_frame_ == the current frame id at entry (one UpdateLocalMap per
 *     frame id).
 * UpdateLocalKeyFrames, quirks included: (1) a slot whose point is bad is cleared (frame_pt_out); (2) every other held point adds one
 * vote to each observer; (3) nobody voted: status = ORBT_ULM_NO_VOTES, local_kf = prev_local_kf unchanged, ref_kf = -1 ("leave
 * reference_keyframe_ alone"); (4) otherwise the voted keyframes that are not bad in ascending kf_rank, marked; (5) ref_kf = the first
 * of them whose count is strictly greater than all before it (:913; -1 when every voted keyframe is bad); (6) the walk of :924-971 over
 * the VOTED keyframes (the reference takes its end iterator before the first append, :924-925, so an appended keyframe is never
 * visited itself): it stops when the size of the growing list is > 80, tested at the top of each iteration; per keyframe the first neighbour that is not
 * bad and not marked, then the first such child, then the parent if it is not marked (isBad() is NOT asked of the parent) - and after
 * a parent the whole walk ends (:968).  A voted list longer than 80 is kept whole.
 * UpdateLocalPoints: over local_kf in order and the slots in order, a point is appended at its first occurrence if it is not bad.
 * SearchLocalPoints' part: mp_state[j] = 0 when the point sits in a slot of frame_pt_out or is in seen_pt, else 1 with pt_nobs > 0,
 * else 3; rows j >= n_local_pt up to cap_pt get mp_state = 0 (their other fields are not written); slot_state[f] = 0 for an empty slot,
 * else 1 / 3 by pt_nobs, slot_Xw[f] = the point's position (zeros for an empty slot).
 *
 * Host pointers, synchronous, one packed upload and one download each.  ORBHIP_EINVAL before any device work for negative counts, CSR
 * offsets that do not ascend from 0, ids out of range, a kf_rank that is not a permutation, more than 10 covisibles in a row, NULL
 * where an array is needed; ORBHIP_ENODEV without a GPU; ORBHIP_ECAP, with only the count written, when a list does not fit.
 * orbt_update_local_keyframes: the graph alone.  votes[nkf] is nullable.                                                            */
#define ORBT_ULM_OK 0
#define ORBT_ULM_NO_VOTES 1
int orbt_update_local_keyframes(int n_kp, const int32_t* frame_pt, int npts, const uint8_t* pt_bad, const int32_t* obs_off, const int32_t* obs_kf, int nkf,
                                const uint8_t* kf_bad, const int32_t* kf_rank, const int32_t* kf_parent, const int32_t* cov_off, const int32_t* cov_kf,
                                const int32_t* child_off, const int32_t* child_kf, int n_prev, const int32_t* prev_local_kf, int cap_kf, int32_t* frame_pt_out,
                                int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf, int32_t* status, int32_t* votes);
/* orbt_update_local_points: its OWN small tables - row i of kf_slot_off[n_local_kf + 1] / kf_slot_pt is the slot table of the i-th
 * local keyframe, the points are numbered by the caller over what those tables and the frame name; frame_pt = the frame's slots (a
 * bad point's slot counts as cleared).  The eight packed outputs mp_Xw[3 cap_pt], mp_normal[3 cap_pt], mp_min_dist, mp_max_dist,
 * mp_desc[32 cap_pt], mp_state[cap_pt], slot_Xw[3 n_kp], slot_state[n_kp] are given all or none; without them pt_nobs and the records
 * may be NULL.                                                                                                                    */
int orbt_update_local_points(int n_local_kf, const int32_t* kf_slot_off, const int32_t* kf_slot_pt, int npts, const uint8_t* pt_bad, const int32_t* pt_nobs,
                             const double* pt_Xw, const double* pt_normal, const float* pt_min_dist, const float* pt_max_dist, const uint8_t* pt_desc, int n_kp,
                             const int32_t* frame_pt, int n_seen, const int32_t* seen_pt, int cap_pt, int32_t* local_pt, int32_t* n_local_pt, double* mp_Xw,
                             double* mp_normal, float* mp_min_dist, float* mp_max_dist, uint8_t* mp_desc, uint8_t* mp_state, double* slot_Xw, uint8_t* slot_state);
/* Both stages over caller-resident DEVICE tables, enqueued on `stream`, no synchronisation inside.  nobs = obs_off[npts], ncov, nchild
 * and nslots = the lengths of the four CSR entry arrays, given by the caller; max_local_slots bounds the slots of the local keyframes
 * together (it sizes the launches: 80 keyframes x their largest slot table, or nslots).  Outputs in caller device buffers:
 * d_frame_pt_out[n_kp] (nullable), d_local_kf[cap_kf], d_local_pt[cap_pt], d_counts[4] = {n_local_kf, ref_kf, n_local_pt, status},
 * d_votes[nkf] (nullable), the eight packed arrays (all or none).  Counts, NULLs and alignment (4 bytes for 32-bit arrays, 16 bytes
 * for the double / descriptor records, the packed outputs and the workspace) are checked on the host; the data is bounds-checked on
 * the device: an entry out of range is treated as absent and sets a bit in *d_status (nullable; zeroed first): 1 = offsets, 2 = index
 * (or kf_rank not a permutation), 4 = n_local_kf > cap_kf, 8 = n_local_pt > cap_pt, 16 = the local keyframes hold more than
 * max_local_slots slots.  With bit 4 or 16 the points stage sees an empty list; with bit 8 every packed row is padding; d_counts keeps
 * the wanted counts and nothing is written beyond a capacity.  A row of cov_kf longer than 10 is walked whole.
 * `d_workspace`: orbt_update_local_map_workspace(...) bytes, 16-byte aligned, not shared with concurrent calls; it is cleared by
 * every call.                                                                                                                     */
int orbt_update_local_map_device(int n_kp, const int32_t* d_frame_pt, int n_seen, const int32_t* d_seen_pt, int n_prev, const int32_t* d_prev_local_kf, int npts,
                                 const uint8_t* d_pt_bad, const int32_t* d_pt_nobs, int nobs, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                 const double* d_pt_Xw, const double* d_pt_normal, const float* d_pt_min_dist, const float* d_pt_max_dist, const uint8_t* d_pt_desc,
                                 int nkf, const uint8_t* d_kf_bad, const int32_t* d_kf_rank, const int32_t* d_kf_parent, int ncov, const int32_t* d_cov_off,
                                 const int32_t* d_cov_kf, int nchild, const int32_t* d_child_off, const int32_t* d_child_kf, int nslots,
                                 const int32_t* d_kf_slot_off, const int32_t* d_kf_slot_pt, int max_local_slots, int cap_kf, int cap_pt, int32_t* d_frame_pt_out,
                                 int32_t* d_local_kf, int32_t* d_local_pt, int32_t* d_counts, int32_t* d_votes, double* d_mp_Xw, double* d_mp_normal,
                                 float* d_mp_min_dist, float* d_mp_max_dist, uint8_t* d_mp_desc, uint8_t* d_mp_state, double* d_slot_Xw, uint8_t* d_slot_state,
                                 uint32_t* d_status, void* d_workspace, void* stream);
/* *bytes = the workspace orbt_update_local_map_device needs (host arithmetic), each section rounded up to 256 bytes: four 32-bit arrays
 * of nkf entries and one of nkf + 1, two of npts, one of max(1, ceil(max_local_slots / 256)) entries (the compaction tiles), 8 bytes. */
int orbt_update_local_map_workspace(int nkf, int npts, int max_local_slots, size_t* bytes);

/* ---- Tracking::TrackReferenceKeyFrame's data-parallel core in one call (src/Tracking.cc:566-615): Frame::ComputeBoW (src/Frame.cc:
 * 322-327, the vocabulary descent), ORBmatcher::SearchByBoW(reference_keyframe_, current_frame_, ...) (src/ORBmatcher.cc:151-256,
 * nnratio 0.7, TH_LOW 50, rotation histogram) and CeresOptimizer::PoseOptimization from last_frame_.Tcw_.
 *   in   img != NULL: the frame is extracted first (as in orbt_track_with_motion_model; kps / desc [cap] receive it) and stays on
 *        the device for a following orbt_track_local_map; img == NULL: the frame an earlier orbt_* call of this thread left there.
 *        Per keyframe feature i < n_kf: descriptor, kf_valid = it holds a map point that is not bad, undistort_keypoints_[i].angle,
 *        the point's position; the keyframe's feature_vector_ as CSR (ascending node ids, as orbv_transform returns it).
 *   out  the frame's BowVector / FeatureVector in orbv_transform's layout (pass NULL for bow_word to skip them);
 *        match_kf[n_kf] = frame feature matched to keyframe feature i or -1; slot_owner[n_kp] = keyframe feature whose map point
 *        current_frame_.map_points_[f] holds, or -1; outlier[n_kp]; res->nmatches (the caller returns false below 15, :582),
 *        pose.  PoseOptimization runs whatever nmatches is.                                                                   */
int orbt_track_reference_keyframe(orbx_ctx* ctx, orbv_ctx* voc, const uint8_t* img, int w, int h, int stride, const float* K4,
                                  const float* bounds, const double* Tcw_last, const uint8_t* kf_desc, const uint8_t* kf_valid,
                                  const float* kf_angle, const double* kf_Xw, int n_kf, const uint32_t* kf_fv_node,
                                  const uint32_t* kf_fv_off, const uint32_t* kf_fv_idx, int kf_fv_n, float nnratio, int check_ori,
                                  orbx_keypoint* kps, uint8_t* desc, int cap, uint32_t* bow_word, double* bow_value, int* n_words,
                                  uint32_t* fv_node, uint32_t* fv_off, uint32_t* fv_idx, int* n_fv_nodes, int32_t* match_kf,
                                  int32_t* slot_owner, uint8_t* outlier, orbt_result* res);

/* ---- lens distortion in the device-resident Tracking calls (configs/EuRoC.yaml, TUM1.yaml, TUM2.yaml).  Once per calibration:
 * orbt_image_bounds + orbt_set_distortion; per frame: the unchanged orbt_* call, then orbt_last_undistorted_keypoints for
 * undistort_keypoints_.  The undistortion is cv::undistortPoints' five fixed-point iterations in double (OpenCV 2.4 / 3.2), the
 * same arithmetic as orbm_undistort_keypoints, bit for bit.
 *
 * Frame::ComputeImageBounds (src/Frame.cc:357-385), host arithmetic: bounds4 = {min_x, max_x, min_y, max_y}.  dist5 = (k1, k2, p1, p2,
 * k3); with dist5[0] == 0 (the reference tests k1 alone) {0, w, 0, h}, otherwise min / max of the four undistorted corners as
 * :374-377 pair them.  ORBHIP_EINVAL for NULL, w <= 0, h <= 0 or non-finite values.                                            */
int orbt_image_bounds(int w, int h, const float* K4, const float* dist5, float* bounds4);
/* Frame::UndistortKeyPoints (src/Frame.cc:329-355) inside every later orbt_* call of the CALLING THREAD that extracts a frame with
 * ctx: the resident frame's records, its grid, the window search, the rotation check and PoseOptimization's observations then use
 * the undistorted coordinates; a keypoint that leaves the grid (PosInGrid false) is in no cell but keeps its slot.  NULL or
 * dist5[0] == 0: none (the default; :330-333).  The state belongs to the thread, not to the context: every thread that extracts
 * with ctx sets it, and a context created later at the same address starts without.  ORBHIP_EINVAL for a NULL context or
 * non-finite coefficients (the state is unchanged then).  The resident frame remembers the coefficients that built it: a call that
 * goes on with it (orbt_track_local_map, img == NULL) after they changed returns ORBHIP_EINVAL - extract a frame first.           */
int orbt_set_distortion(orbx_ctx* ctx, const float* dist5);
/* undistort_keypoints_[i].pt = xy[2 i], xy[2 i + 1] of the frame the calling thread's last extracting orbt_* call produced with ctx
 * (a host copy of what that call downloaded: no device work); the raw coordinates without distortion.  *n = the frame's keypoint
 * count.  ORBHIP_EINVAL without such a frame, ORBHIP_ECAP (only *n written) when cap < *n.                                     */
int orbt_last_undistorted_keypoints(orbx_ctx* ctx, float* xy, int cap, int* n);

/* Host wall time (ms) of the calling thread's most recent orbt_* call, measured inside the library (entry to return): the latency
 * of a Tracking step as the reference's C++ caller would see it, free of what a scripting host adds around the call.       */
double orbt_last_call_ms(void);

/* ------------------------------------------------------------ bundle adjust --
 * Replaces CeresOptimizer::{PoseOptimization, BundleAdjustment/GlobalBundleAdjustemnt,
 * LocalBundleAdjustment, CheckOutlier(s)} (src/CeresOptimizer.cc:49-599) and the Ceres solve
 * underneath (trust-region LM, Huber loss, quaternion manifold, Jacobi scaling; exact Schur
 * solve).  All arithmetic is fp64.  Poses are 7-vectors [tx,ty,tz,qx,qy,qz,qw]
 * (src/MatEigenConverter.cc:66-85); K4 = {fx,fy,cx,cy}.                              */
typedef struct ba_options {
  int32_t max_iterations;      /* options.max_num_iterations */
  double huber_delta;          /* sqrt(5.991) in the reference; applied where obs_robust != 0 */
  int32_t fix_points;          /* 1 = points are constants (PoseOptimization) */
  const volatile uint8_t* stop_flag; /* StopFlagCallback (include/CeresOptimizer.h:332-349); may be NULL.  Any host byte: it is
                                        polled before every enqueue and forwarded to the device while the solve drains, so a flag
                                        raised mid-solve ends it at the next LM iteration boundary with termination 4 and the last
                                        accepted iterate written back */
} ba_options;

/* MatEigenConverter::Matrix4dToMatrix_7_1 / Matrix_7_1_ToMatrix4d (src/MatEigenConverter.cc:66-85): T = row-major 4x4
 * [R t; 0 1] <-> [tx,ty,tz,qx,qy,qz,qw].  Encoding is Eigen::Quaterniond(R).coeffs() (trace / largest-diagonal branches, not
 * normalised); decoding normalises the quaternion first.  Host arithmetic.                                             */
int ba_matrix4d_to_pose7(const double* T, double* pose7);
int ba_pose7_to_matrix4d(const double* pose7, double* T);

typedef struct ba_summary {
  double initial_cost, final_cost;
  int32_t iterations;          /* LM iterations attempted */
  int32_t successful_steps;
  int32_t termination;         /* 0 max-iters 1 gradient 2 parameter 3 function tol 4 user stop 5 failure 6 min-radius
                                  7 device wait timed out (the call returns ORBHIP_ETIMEOUT) */
  double final_radius;
} ba_summary;

/* CeresOptimizer::PoseOptimization(Frame*) (src/CeresOptimizer.cc:275-342) for ONE frame, host pointers.
 * inv_sigma2[i] = frame->inv_level_sigma2s_[octave_i] (used un-square-rooted as in the reference, F7).
 * On return pose7 holds t and the NORMALISED quaternion (":336"), outlier[i] = CheckOutliers flag;
 * *n_inliers = n - n_bad, or 0 with the pose untouched when n < 3 (":330").          */
int ba_pose_optimization(const double* K4, double* pose7, const double* Xw, const double* uv,
                         const float* inv_sigma2, int n, uint8_t* outlier, int* n_inliers, ba_summary* summary);

/* batched, device-resident PoseOptimization: problem p uses observations [offsets[p], offsets[p+1]).
 * d_pose7[np*7] in/out, d_outlier[total], d_n_inliers[np], d_summary[np] (may be NULL). Enqueue only. */
int ba_pose_optimization_batch_device(const double* d_K4 /*np*4*/, double* d_pose7, const double* d_Xw,
                                      const double* d_uv, const float* d_inv_sigma2, const int32_t* d_offsets,
                                      int nproblems, uint8_t* d_outlier, int32_t* d_n_inliers,
                                      ba_summary* d_summary, void* stream);

/* Batches of INDEPENDENT problems (sub-maps) solved in lockstep: every kernel launch covers all problems of
 * the batch (one grid row per problem), each with its own device-side LM state, so small problems fill the 256 CUs together
 * instead of one at a time.  Results are identical to calling the single-problem entry points one by one.               */
typedef struct ba_problem {                 /* arguments of ba_solve */
  const double* K4; double* poses7; const uint8_t* cam_fixed; int32_t ncam;
  double* pts3; int32_t npts;
  const int32_t* obs_cam; const int32_t* obs_pt; const double* obs_uv; const double* obs_weight; const uint8_t* obs_robust;
  int32_t nobs;
} ba_problem;
int ba_solve_batch(const ba_problem* problems, int nproblems, const ba_options* opts, ba_summary* summaries /*[nproblems], may be NULL*/);

typedef struct ba_local_problem {           /* arguments of ba_local_bundle_adjustment */
  const double* K4; double* poses7; const uint8_t* cam_fixed; const uint8_t* cam_local; int32_t ncam;
  double* pts3; int32_t npts;
  const int32_t* obs_cam; const int32_t* obs_pt; const double* obs_uv; const float* obs_inv_sigma2; int32_t nobs;
  uint8_t* obs_erase;                       /* out [nobs] */
} ba_local_problem;
int ba_local_bundle_adjustment_batch(const ba_local_problem* problems, int nproblems, const volatile uint8_t* stop_flag,
                                     int duplicate_blocks, int* aborted, ba_summary* pass1 /*[nproblems] or NULL*/,
                                     ba_summary* pass2 /*[nproblems] or NULL*/);

/* CeresOptimizer::OptimizeSim3(KeyFrame*, KeyFrame*, vector<MapPoint*>& matches12, Sophus::Sim3d& S12, float th2,
 * bool bFixScale) (src/CeresOptimizer.cc:601-735; cost functor include/CeresOptimizer.h:168-236, parameterisation
 * src/CeresOptimizer.cc:24-47) for ONE keyframe pair, host pointers.  Correspondence i (the reference's accepted
 * (map_point_1, map_point_2) pairs, in loop order) carries
 *   P3D2c[i] = R2cw * P3D2w + t2cw, obs1[i] = keyframe_1 keypoint, inv_sigma2_1[i] = kf1->inv_level_sigma2s_[octave]  (:649-664)
 *   P3D1c[i] = R1cw * P3D1w + t1cw, obs2[i] = keyframe_2 keypoint, inv_sigma2_2[i] likewise                         (:666-683)
 * s12[7] in/out = Sophus::Sim3d::data() = [qx,qy,qz,qw (|q|^2 = scale), tx,ty,tz].  th2 -> HuberLoss(sqrt(th2)) and the
 * outlier threshold.  fix_scale is accepted and ignored, as the reference ignores bFixScale.  outlier[n] (may be NULL) =
 * is_outlier_12 || is_outlier_21 (:694-726).  *n_inliers = n - n_bad, or 0 when that is < 10 (:731).                     */
int ba_optimize_sim3(const double* K1 /*fx,fy,cx,cy*/, const double* K2, double* s12, const double* P3D2c,
                     const double* obs1, const float* inv_sigma2_1, const double* P3D1c, const double* obs2,
                     const float* inv_sigma2_2, int n, double th2, int fix_scale, uint8_t* outlier, int* n_inliers,
                     ba_summary* summary);

/* batched, device-resident OptimizeSim3 (one loop candidate per problem): problem p uses correspondences
 * [offsets[p], offsets[p+1]); d_K1/d_K2 [np*4], d_s12 [np*7] in/out, d_th2 [np], d_outlier [total] (may be NULL),
 * d_n_inliers [np], d_summary [np] (may be NULL).  Enqueue only.                                                         */
int ba_optimize_sim3_batch_device(const double* d_K1, const double* d_K2, double* d_s12, const double* d_P3D2c,
                                  const double* d_obs1, const float* d_inv_sigma2_1, const double* d_P3D1c,
                                  const double* d_obs2, const float* d_inv_sigma2_2, const int32_t* d_offsets,
                                  const double* d_th2, int nproblems, uint8_t* d_outlier, int32_t* d_n_inliers,
                                  ba_summary* d_summary, void* stream);

/* CeresOptimizer::OptimizeEssentialGraph (src/CeresOptimizer.cc:737-957), the solve: n_kf Sim(3) vertices given as tangent
 * 7-vectors (Scw.log(), in/out), kf_fixed[v] != 0 for the constant loop keyframe, n_edges EssentialGraphErrorTerm blocks
 * (include/CeresOptimizer.h:266-330) as (vertex j, vertex i, Sji in the qt7 layout) in the reference's insertion order
 * (loop connections :797-821, then per keyframe its parent :839-852, loop edges :855-874 and covisibility edges :877-905;
 * the caller forms Sji = Sjw * Swi from the corrected / non-corrected Sim3 exactly as there).  Identity information, no
 * loss, Sim3Parameterization, <= max_iterations (100 in the reference) LM iterations; the normal equations are solved with
 * the dense FP64-MFMA Cholesky; the reduced system takes (7 n_free)^2 * 8 bytes of device memory (2340 keyframes: 2.1 GB,
 * 10000 keyframes: 39 GB) and ORBHIP_ECAP is returned only when that does not fit.                                         */
int ba_optimize_essential_graph(double* lie7, const uint8_t* kf_fixed, int n_kf, const int32_t* edge_j, const int32_t* edge_i,
                                const double* edge_Sji, int n_edges, int max_iterations, const volatile uint8_t* stop_flag,
                                ba_summary* summary);
/* its write-back arithmetic (:916-956): Tiw[v] = [R | t / s] (row-major 3x4) of exp(lie7_opt[v]); every map point
 * P <- corrected_Swr * (Srw_original * P) with r = pt_ref_kf[p].                                                            */
int ba_essential_graph_correct(const double* lie7_orig, const double* lie7_opt, int n_kf, double* Tiw /*[n_kf*12]*/,
                               const int32_t* pt_ref_kf, double* pts3, int npts);

/* Sophus::Sim3d::exp / log in the layout above (tangent = [upsilon, omega, sigma]); host arithmetic, for bindings that
 * cross the Sophus boundary (LoopClosing builds gScm from (s, R, t): src/LoopClosing.cc:322).                           */
int ba_sim3_exp(const double* tangent7, double* s12_out);
int ba_sim3_log(const double* s12, double* tangent7_out);
/* Sophus::Sim3d::operator* and ::inverse() in the same layout (src/CeresOptimizer.cc:806-813,828-849 form Sji = Sjw * Swi from
 * them; src/LoopClosing.cc:335,458 likewise); out may alias an input.  Host arithmetic.                                   */
int ba_sim3_mul(const double* a, const double* b, double* out);
int ba_sim3_inverse(const double* a, double* out);

/* Measurement hook (no reference counterpart): while enabled, every ba_solve / ba_solve_batch / ba_local_bundle_adjustment(_batch)
 * / call brackets its device work (first kernel .. last LM iteration, copies excluded) with HIP events on the calling thread's
 * stream; ba_get_profile returns the sums of THIS host thread since its last call (device ms, problems solved, LM iterations)
 * and resets them.                                                                                                       */
int ba_set_profiling(int enable);
int ba_get_profile(double* device_ms, int* nsolves, int* lm_iterations);
/* Measurement hook (no reference counterpart): which member of the factorisation family the LAST ba_solve(_batch) /
 * ba_local_bundle_adjustment(_batch) call of THIS host thread took (INTEGRATION.md section 7 has the decision table).  out12 =
 * { problems in the call, look-ahead form (0 none, 1 persistent launch k_chol_persist, 2 one workgroup per system k_chol_wg, 3 one
 * launch per 32-column step k_chol_la), two-level form (0 none, 1 persistent block launches k_chol_persist_blk, 2 hybrid step
 * kernels, 3 classic, 4 one launch), backward substitution (1 k_chol_bsolve_sky, 2 per super-block), largest padded system of the
 * look-ahead family, of the two-level family, widest skyline in 32-column tiles, workgroups of the persistent launch per problem,
 * persistent mode granted by the lease (0 none), a look-ahead system has > 1024 unknowns, every look-ahead system fits k_chol_wg, 0 }. */
int ba_get_last_plan(int32_t* out12);
/* Configuration (no reference counterpart): the time limit, in milliseconds, after which a workgroup of the persistent Cholesky
 * kernels stops waiting for another one and the solve ends with ORBHIP_ETIMEOUT / ba_summary.termination 7 (default 5000 ms;
 * ms <= 0 restores the default; resolution 10 ns).  A deployment with a frame deadline may want tens of milliseconds.  Process-wide,
 * for the default device, for launches made after the call; NOT thread-safe: it synchronises the device - call it at start-up,
 * not while other threads are solving.                                                                                    */
int ba_set_wait_limit_ms(double ms);

/* CeresOptimizer::BundleAdjustment (src/CeresOptimizer.cc:59-225) on flattened arrays, host pointers:
 * cameras with cam_fixed != 0 are constant (KF id 0, fixed KFs); obs_weight multiplies the pixel
 * residual (= invSigma2, F7); obs_robust selects the loss per observation: 0 = none, 1 = Huber, 2 = the observation
 * is present twice, under Huber AND without loss (LocalBA pass 2, F6), folded into one block.  poses7 / pts3 are
 * updated in place with the last accepted iterate (quaternions NOT re-normalised here).             */
int ba_solve(const double* K4_per_cam, double* poses7, const uint8_t* cam_fixed, int ncam, double* pts3,
             int npts, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_uv,
             const double* obs_weight, const uint8_t* obs_robust, int nobs, const ba_options* opts,
             ba_summary* summary);

/* CeresOptimizer::CheckOutlier (src/CeresOptimizer.cc:227-241); host, scalar. depth may be NULL. */
int ba_check_outlier(const double* K4, const double* pose7, const double* Xw, const double* uv,
                     double inv_sigma2, double thres, double* depth);

/* Optimisation core of CeresOptimizer::LocalBundleAdjustment (src/CeresOptimizer.cc:408-598): pass 1
 * Huber / <=5 iterations, outlier classification (chi2 > 5.991 or depth <= 0, local keyframes only),
 * pass 2 with the not-erased observations re-added loss-free ON TOP of pass 1's blocks when
 * duplicate_blocks != 0 (the reference's behaviour) / <=10 iterations, classification again.
 * obs_erase[i] = final to_erase membership.  *aborted = 1 if *stop_flag was set before a solve
 * (nothing written back, ":509-512").  Quaternions are normalised on write-back (":589").         */
int ba_local_bundle_adjustment(const double* K4_per_cam, double* poses7, const uint8_t* cam_fixed,
                               const uint8_t* cam_local, int ncam, double* pts3, int npts,
                               const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_uv,
                               const float* obs_inv_sigma2, int nobs, const volatile uint8_t* stop_flag,
                               int duplicate_blocks, uint8_t* obs_erase, int* aborted, ba_summary* pass1,
                               ba_summary* pass2);

/* ---- multi-GPU: the landmark merge (north_star: "a single RCCL all-gather over xGMI to merge landmark updates") ----
 * One process per GPU, one sub-map per rank; frames and BA sub-problems shard with NO data-path collective.  The one exchange is the
 * merge of the landmark updates after a batched GlobalBA, so that every rank holds the whole map (the reference is one process,
 * src/MonoORBSlam.cc:52-100, src/System.cc: a multi-GPU embedding calls this from the thread that owns the map - LoopClosing's
 * RunGlobalBundleAdjustment, src/LoopClosing.cc:656-740, is where a sub-map's GlobalBA ends).
 * RCCL is looked up at run time (dlopen "librccl.so" or $ORBHIP_RCCL_LIB): liborbslam_hip.so does not link against it.
 *   orbhip_comm_get_unique_id   rank 0 makes the 128-byte id and hands it to the other ranks by whatever the embedding uses (MPI, a file, a socket)
 *   orbhip_comm_create          ncclCommInitRank on `device`; collective: every rank calls it with the same id and world size (<= 64)
 *   orbhip_comm_adopt           wraps an ncclComm_t the caller already owns (not destroyed by orbhip_comm_destroy)
 *   orbhip_allgather_landmarks  ONE ncclAllGather: every rank contributes a slot { count, cap_per_rank x (X, Y, Z[, id]) } - the sub-maps
 *                               are ragged, cap_per_rank is the bound the ranks agree on (ORBHIP_ECAP when n_local exceeds it) - and gets
 *                               the landmarks of all ranks, dense, in rank order: d_pts3_all [cap_all x 3], d_ids_all [cap_all] (NULL on
 *                               both sides when the landmarks carry no ids), counts_out [world size] (host), *n_all = their sum.
 *                               Device pointers; runs on `stream` and synchronises it.  ORBHIP_ECAP when n_all > cap_all.            */
typedef struct orbhip_comm orbhip_comm;
int orbhip_comm_get_unique_id(uint8_t* id128);
int orbhip_comm_create(const uint8_t* id128, int world_size, int rank, int device, orbhip_comm** out);
int orbhip_comm_adopt(void* nccl_comm, int device, orbhip_comm** out);
int orbhip_comm_info(const orbhip_comm* comm, int* world_size, int* rank);
int orbhip_comm_destroy(orbhip_comm* comm);
int orbhip_allgather_landmarks(orbhip_comm* comm, const double* d_pts3_local, const int64_t* d_ids_local, int n_local, int cap_per_rank,
                               double* d_pts3_all, int64_t* d_ids_all, int cap_all, int32_t* counts_out, int* n_all, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBSLAM_HIP_H */
