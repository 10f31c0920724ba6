/* orbline.h -- C ABI of liborbline_hip.so: the MI355X (gfx950) implementation of the per-frame
 * feature path of ORB_Line_SLAM.  Plain pointers and sizes only (no C++/torch types); every entry
 * point names the reference interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - an olf_ctx serves one image size, one parameter block and up to max_images images per call;
 *     a stereo pair is two images: image index = 2*pair + side (0 = left, 1 = right);
 *   - *_dev entry points take DEVICE pointers and enqueue on `stream` (a hipStream_t, NULL = the
 *     context's own stream, a non-blocking one) without synchronising; the others take HOST pointers, copy and
 *     block.  The legacy default stream cannot be named -- its handle IS NULL -- and is not ordered with the
 *     context's streams: a caller that works on it (torch.cuda.current_stream() outside a stream context)
 *     has to synchronise, or work on a stream of its own and pass that;
 *   - per-image outputs are fixed-stride records: image i's key points start at
 *     kps[i * olf_orb_capacity(ctx)], descriptors at desc[i * capacity * 32]; counts[i] says how
 *     many are valid;
 *   - return value: OLF_OK or a negative OLF_ERR_* (orbline_types.h); olf_last_error() gives text.
 *   - a context is not re-entrant; use one per host thread (the reference runs one extractor
 *     object per std::thread, src/Frame.cc:164-171).
 */
#ifndef ORBLINE_H
#define ORBLINE_H

#include "orbline_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct olf_ctx olf_ctx;

/* library / device */
const char* olf_last_error(void);
int olf_device_count(void);                 /* number of visible HIP devices (0 on a CPU-only box) */
/* parameters of Examples/PL/PL_KITTI00-02.yaml:42-55,95-128 + src/Config.cpp:26-160 defaults */
int olf_default_params(olf_params* p);

/* context: replaces constructing ORBextractor x2 + Lineextractor x2 (src/Tracking.cc:131-142) */
/* A context belongs to the device that is current when it is created (calls made with another device current return OLF_ERR_INVALID) and
 * to ONE host thread.  Its scratch buffers are shared by every call, so at most one stream may have work of a context in flight at a time:
 * the *_dev entry points accept any stream, but work enqueued on a second stream must be ordered after the first (event / synchronise) by
 * the caller.
 * Image size: at most 4131 pixels wide and high (FAST candidates are packed with 12 bits per coordinate relative to the 16-pixel border, and the largest
 * coordinate is the side - 36), and large enough that every pyramid level keeps 62 x 62 pixels; anything else is OLF_ERR_INVALID, before any device allocation or
 * launch, and olf_last_error() names which limit was missed.
 * A portrait image -- one whose pyramid has a level with round((w - 32) / (h - 32)) == 0, where ORBextractor's DistributeOctTree divides by zero -- gets a
 * context in which no detector runs: olf_orb_extract*, olf_stereo_points, olf_line_extract* and olf_stereo_frames* return OLF_ERR_INVALID with a message;
 * the entries on caller-supplied key points, key lines and descriptors (olf_lbd_compute among them) serve it. */
int  olf_ctx_create(const olf_params* p, int width, int height, int max_images, olf_ctx** out);
void olf_ctx_destroy(olf_ctx* ctx);
/* Capacity overflows (more corners / key points / segments than a fixed-size device buffer holds) are never silent: the blocking
 * host-pointer entry points return OLF_ERR_CAPACITY themselves; for the asynchronous *_dev entry points the flag is collected by
 * olf_ctx_synchronize (waits for the context's two streams, then reports and clears it) or, without waiting for anything,
 * by olf_ctx_poll_status (call it once the caller's own stream has passed the work in question).  The reference has no such limits
 * (std::vector growth); a refused frame is the equivalent of its std::bad_alloc. */
int  olf_ctx_synchronize(olf_ctx* ctx);
/* Batch pipelining for olf_stereo_frames_dev.  By default the line stream of a call forks from `stream` at the call (the images may have been
 * produced on it), i.e. behind the ORB / stereo / matching tail of the PREVIOUS call on that stream.  With an input event (a hipEvent_t the
 * caller records on whichever stream produces d_images, before the call; NULL = default) the line stream waits for that event only, and the
 * LSD front of batch k + 1 runs beside the tail of batch k.  The context's buffers allow it: the LSD front writes line-path scratch only, and
 * everything of batch k + 1 that touches the output buffers or the shared LBD planes is ordered behind batch k's work on `stream` (api.cpp,
 * olf_stereo_frames_dev).  The caller still orders `stream` itself behind the production of d_images.  The event is ONE-SHOT: the next
 * olf_stereo_frames_dev consumes it (set it again before every call that should use one); the host entry olf_stereo_frames ignores and clears it. */
int  olf_ctx_set_input_event(olf_ctx* ctx, void* hip_event);
/* Deferred join for olf_stereo_frames_dev.  By default the call ends with `stream` waiting for the line stream: every output is complete on `stream`.  The
 * reference's tracker consumes the point features first (TrackReferenceKeyFrame: ComputeBoW + SearchByBoW, src/Tracking.cc:963-970) and the line features after
 * them (:1296-1308); with the deferred join on, the call returns with the ORB-side outputs (key points, descriptors, counts, mvuRight, mvDepth) complete on
 * `stream` and the line-side outputs (key lines, LBD descriptors, line matches) still being produced on the context's line stream --
 * olf_stereo_frames_join_dev(ctx, stream) makes `stream` wait for them (the next olf_stereo_frames_dev call does it itself if the caller did not).
 * A join on the frame call's own stream discharges the obligation for the context; a join on any OTHER stream (explicit, or the implicit one of
 * olf_match_bf_dev / olf_stereo_lines_dev / olf_frames_pack_dev when they are handed a line-side output of the pending call) orders that stream only,
 * and later entries on the frame call's stream still wait.  A kernel of the caller's own that reads line-side outputs must be ordered by the caller
 * (olf_stereo_frames_join_dev on its stream). */
int  olf_ctx_set_deferred_join(olf_ctx* ctx, int on);
int  olf_stereo_frames_join_dev(olf_ctx* ctx, void* stream);
int  olf_ctx_poll_status(olf_ctx* ctx);

/* Stage timing with HIP events recorded on the stream each stage is launched on (the reference's only
 * instrumentation is std::chrono around TrackStereo, Examples/PL/PL_stereo_kitti.cc:80-97).  Accumulates
 * per-stage total milliseconds and call counts while enabled; read/reset synchronise the device. */
int olf_profile_enable(olf_ctx* ctx, int on);
int olf_profile_reset(olf_ctx* ctx);
int olf_profile_stage_count(void);
const char* olf_profile_stage_name(int stage);
int olf_profile_read(olf_ctx* ctx, double* total_ms, int32_t* calls);   /* arrays of olf_profile_stage_count() */

/* ---- input conditioning ahead of the path ------------------------------------------------- */
enum { OLF_RGB2GRAY = 0, OLF_BGR2GRAY = 1, OLF_RGBA2GRAY = 2, OLF_BGRA2GRAY = 3 };
/* cv::cvtColor(img, gray, CV_*2GRAY) of Tracking::GrabImageStereo (src/Tracking.cc:193-218): n_images interleaved 8-bit
 * images (3 or 4 channels) of the context's size -> n_images gray images.  Device pointers. */
int olf_cvt_gray_dev(olf_ctx* ctx, const uint8_t* d_src, int code, int n_images, uint8_t* d_gray, void* stream);
/* cv::remap(src, dst, M1, M2, INTER_LINEAR) with two CV_32FC1 maps and BORDER_CONSTANT 0, the EuRoC rectification of
 * Examples/PL/PL_stereo_euroc.cc:136-137.  src: n_images images src_w x src_h (stride src_w); maps: dst_w*dst_h floats each
 * (shared by all images, e.g. one call per camera); dst: n_images images dst_w x dst_h.  Device pointers. */
int olf_remap_linear_dev(olf_ctx* ctx, const uint8_t* d_src, int src_w, int src_h, const float* d_mapx, const float* d_mapy, int dst_w,
                         int dst_h, int n_images, uint8_t* d_dst, void* stream);
/* cv::initUndistortRectifyMap(K, D, R, P(3x3), Size(w, h), CV_32F, M1, M2), Examples/PL/PL_stereo_euroc.cc:97-98: the two CV_32FC1 maps
 * olf_remap_linear takes.  K, R, P: 3 x 3 row-major doubles (P = the left 3 x 3 block of the projection matrix); D: n_dist <= 8 distortion
 * coefficients in OpenCV's order k1 k2 p1 p2 k3 k4 k5 k6.  Double arithmetic in the order of OpenCV 3.4's generic code (convention C.13). */
int olf_init_undistort_rectify_map_dev(olf_ctx* ctx, const double* K, const double* D, int n_dist, const double* R, const double* P, int w, int h,
                                       float* d_map1, float* d_map2, void* stream);
int olf_init_undistort_rectify_map(olf_ctx* ctx, const double* K, const double* D, int n_dist, const double* R, const double* P, int w, int h,
                                   float* map1, float* map2);
/* host-buffer forms (copy, run, copy back, block) */
int olf_cvt_gray(olf_ctx* ctx, const uint8_t* src, int code, int n_images, uint8_t* gray);
int olf_remap_linear(olf_ctx* ctx, const uint8_t* src, int src_w, int src_h, const float* mapx, const float* mapy, int dst_w, int dst_h,
                     int n_images, uint8_t* dst);

/* ---- MapPoint / MapLine::ComputeDistinctiveDescriptors (src/MapPoint.cc:254-318, src/MapLine.cc:257-322) --
 * n_points landmarks; landmark p is observed by descriptors desc[offs[p] .. offs[p+1]) (32 bytes each, the rows the reference gathers
 * from the non-bad key frames, in its std::map iteration order).  best[p] = index inside that list of the descriptor with the least
 * median distance to the others (first minimum), -1 for an empty list.  Host buffers; at most 1024 observations per landmark. */
int olf_distinctive_descriptors(olf_ctx* ctx, const uint8_t* desc, const int32_t* offs, int n_points, int32_t* best);

/* ---- key-frame feature record of the binary map file -----------------------------------------
 * void Map::SaveKeyFrame(ofstream &f, KeyFrame* kf), src/Map.cc:283-373 / KeyFrame* Map::LoadKeyFrame(ifstream &f, ...), :376-531,
 * for the members the feature path produces: byte-exact what f.write((char*)&member, sizeof(member)) writes member by member.
 * Host code (no device needed), like the reference's.  *_ids: NULL = no MapPoint / MapLine anywhere (ULONG_MAX is written). */
size_t olf_kf_record_bytes(int n_keys, int n_lines);
int olf_kf_record_pack(uint64_t frame_id, uint64_t kf_id, double timestamp, const float* t3, const float* quat4, int n_keys,
                       const olf_keypoint* keys, const float* uright, const float* depth, const uint8_t* desc, const uint64_t* mappoint_ids,
                       int n_lines, const olf_keyline* lines, const float* disparity2, const double* le3, const uint8_t* ldesc,
                       const uint64_t* mapline_ids, uint8_t* out, size_t capacity, size_t* written);
int olf_kf_record_counts(const uint8_t* buf, size_t len, int32_t* n_keys, int32_t* n_lines, size_t* record_bytes);
int olf_kf_record_unpack(const uint8_t* buf, size_t len, uint64_t* frame_id, uint64_t* kf_id, double* timestamp, float* t3, float* quat4,
                         olf_keypoint* keys, float* uright, float* depth, uint8_t* desc, uint64_t* mappoint_ids, olf_keyline* lines,
                         float* disparity2, double* le3, uint8_t* ldesc, uint64_t* mapline_ids);

/* ---- BoW transform: ORBVocabulary / LineVocabulary (include/ORBVocabulary.h:30-34) ----------
 * = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>; transform() is called by Frame::ComputeBoW (src/Frame.cc:585-597) and
 * KeyFrame::ComputeBoW (src/KeyFrame.cc:96-112) with levelsup = 4. */
typedef struct olf_voc olf_voc;
/* scoring: 0 L1_NORM 1 L2_NORM 2 CHI_SQUARE 3 KL 4 BHATTACHARYYA 5 DOT_PRODUCT; weighting: 0 TF_IDF 1 TF 2 IDF 3 BINARY
 * (Thirdparty/DBoW2/DBoW2/BowVector.h:36-53).  Nodes in id order (node 0 = root, entry ignored): parent[i] < i, is_leaf[i] marks a
 * word (word ids are assigned in node order), desc 32 bytes per node, weight per node.  The tree is uploaded to the current device. */
int olf_voc_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                   const double* weight, olf_voc** out);
/* TemplatedVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1425): "k L scoring weighting" then one
 * "parent isLeaf d0..d31 weight" line per node. */
int olf_voc_load_text(const char* path, olf_voc** out);
void olf_voc_destroy(olf_voc* voc);
int olf_voc_info(const olf_voc* voc, int* k, int* L, int* scoring, int* weighting, int* n_nodes, int* n_words);
/* transform(feature, word_id, weight, nid, levelsup) (:1217-1261) for n descriptors; device pointers. */
int olf_bow_words_dev(olf_ctx* ctx, const olf_voc* voc, const uint8_t* d_desc, int n, int levelsup, int32_t* d_word, double* d_weight,
                      int32_t* d_node, void* stream);
/* host: per-feature (word, weight, node) -> BowVector (ascending word id) + FeatureVector (CSR over ascending node id), with the
 * vocabulary's weighting / normalisation (:1127-1195, BowVector.cpp:34-84, FeatureVector.cpp:31-45).  Capacities: n (fv_offs n+1). */
int olf_bow_assemble(const olf_voc* voc, const int32_t* word, const double* weight, const int32_t* node, int n, int32_t* bow_ids,
                     double* bow_vals, int* n_bow, int32_t* fv_nodes, int32_t* fv_offs, int32_t* fv_idx, int* n_fv);
/* transform(features, v, fv, levelsup) for one image's descriptors (host buffers): descent on the GPU, assembly on the host. */
int olf_bow_transform(olf_ctx* ctx, const olf_voc* voc, const uint8_t* desc, int n, int levelsup, int32_t* bow_ids, double* bow_vals,
                      int* n_bow, int32_t* fv_nodes, int32_t* fv_offs, int32_t* fv_idx, int* n_fv);
/* Batched, device-resident ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBmatcher.cc:161-290,
 * Tracking::TrackReferenceKeyFrame, src/Tracking.cc:963-970) over consecutive frames, Frame::ComputeBoW (src/Frame.cc:585-597) of every frame
 * included -- no host step between a frame's descriptors and its matches.  Frame j = image j * img_stride of the key point / descriptor / count
 * buffers of olf_orb_extract_dev (stride olf_orb_capacity(); img_stride 2 = the left images of a stereo batch); pair j: pKF = frame j, F = frame
 * j + 1, j < n_frames - 1.  d_mp_valid / d_mp_bad [n_frames][capacity] bytes: vpMapPointsKF[i] != NULL / isBad() of a frame in its key-frame
 * role (NULL: every feature holds a good map point).  levelsup: 4 in the reference.  d_matches [n_frames - 1][capacity]: per feature of F the
 * index of the pKF feature whose map point it received (-1 = NULL); d_nmatches [n_frames - 1] = the reference's return values.  The greedy
 * state of the reference (a feature of F that holds a match is skipped, :214) is kept: inside a vocabulary node the key frame's features are
 * walked in order by one wave; different nodes share no feature and run side by side. */
int olf_search_by_bow_batch_dev(olf_ctx* ctx, const olf_voc* voc, int n_frames, int img_stride, const olf_keypoint* d_kps, const uint8_t* d_desc,
                                const int32_t* d_counts, const uint8_t* d_mp_valid, const uint8_t* d_mp_bad, float nnratio, int check_orientation,
                                int levelsup, int32_t* d_matches, int32_t* d_nmatches, void* stream);

/* ---- ORBextractor (include/ORBextractor.h:52-118, src/ORBextractor.cc) -------------------- */
/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (include/ORBextractor.h:68-91) + mnFeaturesPerLevel; arrays of nlevels */
int olf_orb_scale_tables(const olf_ctx* ctx, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                         int32_t* features_per_level);
/* level sizes of mvImagePyramid (src/ORBextractor.cc:1113-1114) */
int olf_orb_level_sizes(const olf_ctx* ctx, int32_t* widths, int32_t* heights);
/* per-image capacity of the key point / descriptor records */
int olf_orb_capacity(const olf_ctx* ctx);
/* ORBextractor::operator()(image, mask [ignored], keypoints, descriptors), src/ORBextractor.cc:1045-1107,
 * for n_images images of width x height, row stride = width. */
/* one image whose rows are row_stride bytes apart (a cv::Mat ROI: data, step) -- no host-side repacking */
int olf_orb_extract_strided(olf_ctx* ctx, const uint8_t* image, size_t row_stride, olf_keypoint* kps, uint8_t* desc, int32_t* count);
int olf_orb_extract_dev(olf_ctx* ctx, const uint8_t* d_images, int n_images, olf_keypoint* d_kps, uint8_t* d_desc,
                        int32_t* d_counts, void* stream);
int olf_orb_extract(olf_ctx* ctx, const uint8_t* images, int n_images, olf_keypoint* kps, uint8_t* desc, int32_t* counts);
/* read back mvImagePyramid[level] of image `image` of the last extract call (public member of the
 * reference class, read by Frame::ComputeStereoMatches src/Frame.cc:799-816).  blurred != 0 returns
 * the GaussianBlur'ed working image of src/ORBextractor.cc:1087-1088 instead.  dst: w*h bytes. */
int olf_orb_pyramid_level(olf_ctx* ctx, int image, int level, int blurred, uint8_t* dst);
/* debug/test: per-level FAST candidates handed to DistributeOctTree (vToDistributeKeys,
 * src/ORBextractor.cc:821-827) as int32 triples (x,y,score) relative to minBorder. */
int olf_orb_debug_candidates(olf_ctx* ctx, int image, int level, int32_t* xys, int cap, int32_t* count);
/* debug/test, host only (no context, no device): the launches of the octree kernel for these parameters and this image size.  Returns their number (1 to 3)
 * or an error; level_launch [nlevels] = the launch a level goes in, launch_lds [3] = the dynamic LDS bytes each launch asks for (-1: no such launch; 0: the
 * one launch of a configuration whose lists live in global memory). */
int olf_debug_octree_launches(const olf_orb_params* params, int width, int height, int32_t* level_launch, int32_t* launch_lds);
/* debug: the context's 64-int device status block (overflow flags in [0]; instrumented builds put cycle counters at [16..31]). */
int olf_debug_status(olf_ctx* ctx, int32_t* out64);
int olf_debug_status_n(olf_ctx* ctx, int32_t* out, int n);
/* debug: the regions the last LSD growth logged for `image`, in detection order: (list start, pixel count) pairs and final region angles */
int olf_debug_lsd_owner(olf_ctx* ctx, int image, uint32_t* out);      /* debug: owner words of the last growth, Ws*Hs */
int olf_debug_lsd_regions(olf_ctx* ctx, int image, int32_t* start_n, double* angle, int cap, int32_t* count);     /* the first n (<= 256) words */
/* debug/test: waves per image of the LSD region-growing kernel (1..16; 0 = the one-wave sequential agent; -1 = automatic from the batch
 * size) and entries of its reorder buffer (128, 256, 512, or 1024 with several workgroups per image; 0 = automatic).  Results do not depend on either. */
int olf_debug_lsd_waves(olf_ctx* ctx, int waves_per_image, int rob_entries);
/* debug/test: workgroups (CUs) that grow ONE image together when the kernel runs 16 waves per image (1, 2 or 4; 0 = automatic from the batch
 * size: calls of up to 64 images -- the one-pair-per-call shape of Frame::Frame, src/Frame.cc:164-171 -- take 2).  Results do not depend on it. */
int olf_debug_lsd_groups(olf_ctx* ctx, int groups);
/* debug/test: where the groups of an image run.  0 (default): on workgroups 8 apart, which the hardware's round-robin placement puts on ONE XCD (they
 * meet in its L2); 1: on consecutive workgroups, i.e. on DIFFERENT XCDs.  What crosses between groups is agent-scope traffic either way: results do
 * not depend on it (tests/test_lsd_grow_gpu.py::test_growth_groups_scattered_over_xcds), only the time does. */
int olf_debug_lsd_scatter(olf_ctx* ctx, int on);
/* debug/test: cap the primary pixel log of the one-wave region growing at `entries` pixels per image (0 = the context's own capacity: every pixel in
 * contexts of up to 2048 images, half of the pixels in larger -- batch -- contexts).  Images that log more are grown again on a block of the context's spill
 * arena inside the same call; when the arena is exhausted the call reports OLF_ERR_CAPACITY.  Results do not depend on it. */
int olf_debug_lsd_log_cap(olf_ctx* ctx, int entries);
/* debug / tests: the kernel that replays libstdc++'s std::sort for the LSD seed order (convention C.9 variant 1, csrc/lsd_seedsort.hip) on a
 * caller-supplied array of n <= Ws*Hs keys, (field << 22) | payload with a 10-bit field: out receives the keys whose field is <= kthr in the
 * order std::sort(keys, keys + n, field ascending) leaves them; depth_limit < 0 = introsort's own 2 * floor(log2 n), a small value forces
 * its heap-sort branch. */
int olf_debug_seed_sort(olf_ctx* ctx, const uint32_t* keys, int n, int kthr, int depth_limit, uint32_t* out, int32_t* out_n);
/* debug / tests: the kernel variant of that replay -- 0: one wave per image (batches), 1 / 2: 4 / 8 cooperating waves per image (few images: the
 * drop-in's one-pair-per-call shape), 5: 2 waves per image, -1: chosen from the batch size; 3 and 4 are rejected (OLF_ERR_INVALID).  Results do not
 * depend on it. */
int olf_debug_seed_sort_mode(olf_ctx* ctx, int mode);
/* debug / tests: the seed-order kernel of the capacity path (csrc/lsd_wide.hip: lsd_n_bins > 1024 or an LSD working image of 2^22 pixels and more -- free YAML
 * keys of the reference, src/Config.cpp:268,274) on a caller-supplied array of 64-bit keys (field << 32 | payload).  full = 0: the order libstdc++'s
 * std::sort(begin, end, field ascending) leaves (convention C.9 variant 1, OpenCV lsd.cpp ll_angle); full = 1: ascending whole words (variant 0).  Keys whose
 * field is <= kthr are listed: out receives their payloads in order, *out_n their number.  depth_limit: introsort's depth limit (-1: 2 * floor(log2 n)).  The
 * context must be a wide one. */
int olf_debug_seed_sort_wide(olf_ctx* ctx, const uint64_t* keys, int n, int64_t kthr, int depth_limit, int full, uint32_t* out, int32_t* out_n);
/* debug / tests: cap the 32-pixel chunk pool the multi-wave growth may use per image (0: all of it).  An image that exhausts the pool is grown
 * again by the one-wave agent inside the same call -- the result does not change, only the time. */
int olf_debug_lsd_pool(olf_ctx* ctx, int pool_chunks);
/* debug/test: the LSD agent's unscaled exact float division against IEEE division on blocks*256*per_thread pseudo-random operand pairs
 * from its operand range; *mismatches = number of quotients that differ in any bit (must be 0). */
int olf_debug_fdiv_sweep(olf_ctx* ctx, uint64_t seed, int blocks, int per_thread, uint64_t* mismatches);
/* debug/test: the lean sqrt(n / 4.0) of the LSD key kernel (ll_angle's gradient norm; lsd_device.hpp sqrt_quarter) against the compiler's IEEE
 * sqrt on every integer n in [0, count); *mismatches = number of results that differ in any bit (must be 0). */
int olf_debug_sqrtq_sweep(olf_ctx* ctx, int count, uint64_t* mismatches);
/* debug/test: the growth agent's cheap alignment test (dot / cross products of the region's float sums with a candidate's tabulated direction, decided under a
 * margin that bounds cv::fastAtan2's error -- csrc/lsd.hip, PF bit 16) against the reference's expression |fastAtan2(sums) * DEG2RAD - angle| <= prec
 * (OpenCV lsd.cpp isAligned as called by region_grow; LSDDetector_custom.cpp:246,262) on blocks*256*per_thread pseudo-random (sums, candidate) pairs, three
 * quarters of them within 3 mrad of the tolerance: out3[0] = certain decisions that contradict the reference (must be 0), out3[1] = decisions left to the
 * reference's expression, out3[2] = all. */
int olf_debug_align_sweep(olf_ctx* ctx, uint64_t seed, int blocks, int per_thread, uint64_t* out3);

/* ---- Frame::ComputeStereoMatches (src/Frame.cc:702-876) ------------------------------------- */
/* Stereo point matching for n_pairs pairs whose ORB features (images 2p = left, 2p+1 = right) came from
 * the immediately preceding olf_orb_extract*_dev call on this context (its device-resident
 * mvImagePyramid of both extractors is read for the 11x11 SAD refinement, src/Frame.cc:799-816).
 * Outputs per pair, stride olf_orb_capacity(): mvuRight / mvDepth (-1 = no match), src/Frame.cc:704-705.
 * The key points may be the caller's own (the buffers are read, only the pyramids come from the extractor call), as long as every SAD window
 * stays inside its level as the extractor's would.  A context whose olf_orb_capacity() exceeds 32768 is refused with OLF_ERR_CAPACITY before
 * anything is launched: the row sort and the median sort hold one image's keys in LDS. */
int olf_stereo_points_dev(olf_ctx* ctx, int n_pairs, const olf_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_counts,
                          float* d_uright, float* d_depth, void* stream);
/* host convenience: ExtractORB x2 + ComputeStereoMatches for n_pairs pairs (images: 2*n_pairs) */
int olf_stereo_points(olf_ctx* ctx, const uint8_t* images, int n_pairs, olf_keypoint* kps, uint8_t* desc, int32_t* counts,
                      float* uright, float* depth);

/* ---- LineMatcher / ORBmatcher brute force (src/LineMatcher.cpp:42-62,104-132; App. A.10) ------- */
/* match(desc1, desc2, nnr, matches_12) for n_sets independent sets: set s has d_nA[s*a_step] rows at
 * d_descA + s*strideA*32 and d_nB[s*b_step] rows at d_descB + s*strideB*32.  kNN(2) both ways, ratio
 * test d0 < d1*nnr, mutual check when best_lr (Config::bestLRMatches()).  d_m12: n_sets*strideA ints,
 * -1 = no match. */
int olf_match_bf_dev(olf_ctx* ctx, const uint8_t* d_descA, const int32_t* d_nA, int strideA, int a_step, const uint8_t* d_descB,
                     const int32_t* d_nB, int strideB, int b_step, int n_sets, float nnr, int best_lr, int32_t* d_m12, void* stream);
int olf_match_bf(olf_ctx* ctx, const uint8_t* descA, int nA, const uint8_t* descB, int nB, float nnr, int best_lr, int32_t* m12);
/* cv::BFMatcher(NORM_HAMMING).knnMatch(k=2) (host buffers): per query best index, best and second distance
 * (-1 / INT_MAX where the train set is too small) */
int olf_knn2(olf_ctx* ctx, const uint8_t* descQ, int nQ, const uint8_t* descT, int nT, int32_t* idx0, int32_t* dist0, int32_t* dist1);
/* Candidate-list distances for ORBmatcher::SearchByProjection (src/ORBmatcher.cc:1330-1472) / SearchByBoW (:161-290):
 * query i is compared with train rows cand_idx[cand_offsets[i] .. cand_offsets[i+1]) (CSR, built by the caller from
 * Frame::GetFeaturesInArea -- on the device: olf_features_in_area_dev -- / the BoW feature vectors); dist[k] receives the Hamming distance of pair k (0xffff for an
 * out-of-range index).  The order-dependent greedy resolution stays with the caller. */
int olf_match_candidates_dev(olf_ctx* ctx, const uint8_t* d_descQ, int nQ, const uint8_t* d_descT, int nT, const int32_t* d_cand_offsets,
                             const int32_t* d_cand_idx, uint16_t* d_dist, void* stream);
int olf_match_candidates(olf_ctx* ctx, const uint8_t* descQ, int nQ, const uint8_t* descT, int nT, const int32_t* cand_offsets,
                         const int32_t* cand_idx, uint16_t* dist);
/* ---- the per-frame ORBmatcher searches, complete (host candidate generation + GPU distances + the reference's resolution) ----
 * Plain view of the Frame / KeyFrame members these searches read (include/Frame.h:49-260, include/KeyFrame.h).  Pointers a search
 * does not read may be NULL.  mp_valid / mp_obs stand for `mvpMapPoints[i] != NULL` and `mvpMapPoints[i]->Observations() > 0`; the
 * searches that assign map points to the current frame update them in place, as the reference updates mvpMapPoints.
 * Constness: the entry points take `const olf_frame_view*` -- the VIEW (its pointers and counts) is never modified; mp_valid and mp_obs are
 * deliberately pointers to non-const bytes, because for the current frame they are outputs (each function's comment names what it updates).
 * Every other array is read-only.  A supplied grid (grid_offsets / grid_index) is checked in O(OLF_GRID_CELLS + n) before a search walks it --
 * offsets monotone from 0, the last one <= n, indices in [0, n) -- and a grid that fails is OLF_ERR_INVALID. */
typedef struct olf_frame_view {
    const olf_keypoint* keys;     /* mvKeysUn (= mvKeys for a rectified camera, src/Frame.cc:601-605)            */
    const uint8_t* desc;          /* mDescriptors [n][32]                                                        */
    const float*   uright;        /* mvuRight [n] (negative = monocular point)                                   */
    int32_t        n;             /* N                                                                           */
    uint8_t*       mp_valid;      /* [n]                                                                         */
    uint8_t*       mp_obs;        /* [n]                                                                         */
    const uint8_t* mp_bad;        /* [n] pMP->isBad()                                                            */
    const float*   mp_world;      /* [n][3] pMP->GetWorldPos()                                                   */
    const uint8_t* mp_desc;       /* [n][32] pMP->GetDescriptor()                                                */
    const uint8_t* outlier;       /* [n] mvbOutlier                                                              */
    const float*   Tcw;           /* mTcw, 4x4 row-major                                                         */
    float fx, fy, cx, cy, mbf, minX, maxX, minY, maxY;     /* calibration, mnMinX .. mnMaxY                      */
    const float*   scale_factors; /* mvScaleFactors [n_levels]                                                   */
    int32_t        n_levels;
    const float*   mp_maxd;       /* [n] pMP->mfMaxDistance (key-frame searches that predict a scale level)      */
    const float*   mp_mind;       /* [n] pMP->mfMinDistance                                                      */
    const int32_t* fv_nodes;      /* mFeatVec (DBoW2::FeatureVector) as CSR: ascending node ids [fv_n],          */
    const int32_t* fv_offsets;    /*   offsets [fv_n + 1],                                                       */
    const int32_t* fv_features;   /*   feature indices                                                           */
    int32_t        fv_n;
    const int32_t* grid_offsets;  /* mGrid, prebuilt (olf_frame_grid; layout in orbline_types.h): [OLF_GRID_CELLS + 1] and              */
    const int32_t* grid_index;    /*   [grid_offsets[OLF_GRID_CELLS]], host pointers.  NULL: the search builds the grid from `keys` itself */
} olf_frame_view;
/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono), src/ORBmatcher.cc:1330-1472
 * (Tracking::TrackWithMotionModel, every frame).  matches[i2] = index of the LastFrame feature whose map point CurrentFrame feature i2
 * received (-1 = none); cur->mp_valid / mp_obs are updated; *nmatches = the reference's return value. */
int olf_search_by_projection(olf_ctx* ctx, const olf_frame_view* cur, const olf_frame_view* last, float th, int bMono, int check_orientation,
                             int32_t* matches, int32_t* nmatches);
/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono, map<int,int>& match12),
 * src/ORBmatcher.cc:1474-1618 -- the overload Tracking::TrackWithMotionModelWithLine calls (src/Tracking.cc:1296,1302).  Same search; match12[i2]
 * = the value the reference's map holds under key i2 (-1: no such key): match12.insert keeps the FIRST LastFrame index CurrentFrame feature i2
 * was matched with (:1577) while matches[i2] / mvpMapPoints[i2] keep the last one (:1575); match12.erase on a rotation rejection (:1612).
 * Walking i2 upwards over match12[i2] >= 0 reproduces the map's iteration order. */
int olf_search_by_projection_match12(olf_ctx* ctx, const olf_frame_view* cur, const olf_frame_view* last, float th, int bMono, int check_orientation,
                                     int32_t* matches, int32_t* match12, int32_t* nmatches);
/* int ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched, vector<int> &vnMatches12, int windowSize),
 * src/ORBmatcher.cc:407-522 (monocular map initialisation).  Only keys / desc / n / the image bounds of the views are read.
 * prev_matched: f1->n (x, y) pairs, updated in place with the matched F2 positions; matches12[i1] = F2 index or -1. */
int olf_search_for_initialization(olf_ctx* ctx, const olf_frame_view* f1, const olf_frame_view* f2, float* prev_matched, int window_size,
                                  float nnratio, int check_orientation, int32_t* matches12, int32_t* nmatches);
/* int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches), src/ORBmatcher.cc:161-290
 * (Tracking::TrackReferenceKeyFrame / Relocalization).  matched[iF] = index of the key-frame feature whose map point feature iF of F
 * received (-1 = none). */
int olf_search_by_bow(olf_ctx* ctx, const olf_frame_view* kf, const olf_frame_view* f, float nnratio, int check_orientation, int32_t* matched,
                      int32_t* nmatches);
/* int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th), src/ORBmatcher.cc:47-131
 * (Tracking::SearchLocalPoints, every frame).  Map point members as arrays of n_mp: mbTrackInView, isBad(), mnTrackScaleLevel,
 * mTrackViewCos, (mTrackProjX, mTrackProjY, mTrackProjXR) interleaved, GetDescriptor(), Observations() > 0.
 * matches[idx] = index into vpMapPoints given to feature idx of F (-1 = none); f->mp_valid / mp_obs are updated. */
int olf_search_local_map(olf_ctx* ctx, const olf_frame_view* f, int n_mp, const uint8_t* track_in_view, const uint8_t* bad,
                         const int32_t* track_scale_level, const float* track_view_cos, const float* track_proj3, const uint8_t* mp_desc,
                         const uint8_t* mp_obs, float th, float nnratio, int32_t* matches, int32_t* nmatches);

/* bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit), src/Frame.cc:388-444, for n_mp map points at once (host arithmetic, no
 * device work): the producer of olf_search_local_map's inputs in Tracking::SearchLocalPoints (src/Tracking.cc:1900-1945).  f supplies mTcw,
 * the calibration, the image bounds and mvScaleFactors.  Outputs per point: mbTrackInView, mnTrackScaleLevel, mTrackViewCos and
 * (mTrackProjX, mTrackProjY, mTrackProjXR); a point that fails a gate only gets track_in_view = 0. */
int olf_is_in_frustum(const olf_frame_view* f, int n_mp, const float* world, const float* normal, const float* maxd, const float* mind,
                      float viewing_cos_limit, uint8_t* track_in_view, int32_t* track_scale_level, float* track_view_cos, float* track_proj3);

/* ---- the LocalMapping / LoopClosing / relocalisation searches, same split (host candidates, GPU distances, host resolution) ----
 * int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th,
 * const int ORBdist), src/ORBmatcher.cc:1620-1747.  already_found[i] = sAlreadyFound.count(pKF's i-th map point) (may be NULL);
 * matches[i2] = key-frame feature whose map point CurrentFrame feature i2 received; cur->mp_valid is updated. */
int olf_search_by_projection_kf(olf_ctx* ctx, const olf_frame_view* cur, const olf_frame_view* kf, const uint8_t* already_found, float th,
                                int orb_dist, int check_orientation, int32_t* matches, int32_t* nmatches);
/* int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12), src/ORBmatcher.cc:524-657.
 * matches12[idx1] = feature of pKF2 whose map point is taken (-1 = NULL). */
int olf_search_by_bow_kf(olf_ctx* ctx, const olf_frame_view* kf1, const olf_frame_view* kf2, float nnratio, int check_orientation,
                         int32_t* matches12, int32_t* nmatches);
/* int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs,
 * const bool bOnlyStereo), src/ORBmatcher.cc:659-825.  F12 3x3 row-major; Cw = pKF1->GetCameraCenter() (NULL: derived from kf1->Tcw).
 * matches12[idx1] = idx2 (-1 = none): vMatchedPairs is the list of (idx1, matches12[idx1]) in idx1 order. */
int olf_search_for_triangulation(olf_ctx* ctx, const olf_frame_view* kf1, const olf_frame_view* kf2, const float* F12, const float* Cw,
                                 int only_stereo, int check_orientation, int32_t* matches12, int32_t* nmatches);
/* The search part of int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th), src/ORBmatcher.cc:827-948:
 * per map point (skip = !pMP || isBad() || IsInKeyFrame(pKF); world, normal, mfMaxDistance, mfMinDistance, descriptor) the most similar key
 * point inside the projection window: best_idx / best_dist (-1 / 256 where a gate rejects the point).  Ow = pKF->GetCameraCenter()
 * (NULL: derived from kf->Tcw).  The reference then fuses when best_dist <= TH_LOW (:950-972, map mutation, host code). */
int olf_fuse_search(olf_ctx* ctx, const olf_frame_view* kf, int n_mp, const uint8_t* skip, const float* world, const float* normal,
                    const float* maxd, const float* mind, const uint8_t* desc, float th, const float* Ow, int32_t* best_idx, int32_t* best_dist);
/* The search part of int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*>
 * &vpReplacePoint), src/ORBmatcher.cc:977-1102 (Scw 4x4 row-major; skip = isBad() || spAlreadyFound.count(pMP)); best_dist is INT_MAX
 * where nothing was found. */
int olf_fuse_search_sim3(olf_ctx* ctx, const olf_frame_view* kf, const float* Scw, int n_mp, const uint8_t* skip, const float* world,
                         const float* normal, const float* maxd, const float* mind, const uint8_t* desc, float th, int32_t* best_idx,
                         int32_t* best_dist);
/* int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th),
 * src/ORBmatcher.cc:292-405 (LoopClosing::ComputeSim3, src/LoopClosing.cc:381): the loop candidate's map points projected into the key frame
 * under the Sim3 pose Scw (4x4, row-major).  skip[i] = vpPoints[i]->isBad() || spAlreadyFound.count(vpPoints[i]) (:311-312, :321); the point
 * arrays as in olf_fuse_search_sim3.  matched[idx] (in / out, kf->n bytes) = vpMatched[idx] != NULL: a key point that holds a match is passed
 * over (:378) and a point whose best distance is <= TH_LOW takes its key point at once (:397-401) -- matches[idx] = the index into vpPoints
 * key point idx received in this call (-1 = none); *nmatches = the reference's return value. */
int olf_search_by_projection_sim3(olf_ctx* ctx, const olf_frame_view* kf, const float* Scw, int n_mp, const uint8_t* skip, const float* world,
                                  const float* normal, const float* maxd, const float* mind, const uint8_t* desc, float th, uint8_t* matched,
                                  int32_t* matches, int32_t* nmatches);
/* int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12,
 * const cv::Mat &t12, const float th), src/ORBmatcher.cc:1104-1328.  matches12[i1]: in -- -1 = NULL, >= 0 = pMP->GetIndexInKeyFrame(pKF2),
 * -2 = a map point pKF2 does not observe; out -- additionally the agreed matches.  vn_match1 / vn_match2 = vnMatch1 / vnMatch2. */
int olf_search_by_sim3(olf_ctx* ctx, const olf_frame_view* kf1, const olf_frame_view* kf2, int32_t* matches12, float s12, const float* R12,
                       const float* t12, float th, int32_t* vn_match1, int32_t* vn_match2, int32_t* nfound);

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1795-1811) over all pairs: out[nA][nB] uint16 (host buffers) */
int olf_hamming_matrix(olf_ctx* ctx, const uint8_t* descA, int nA, const uint8_t* descB, int nB, uint16_t* out);

/* ---- Lineextractor (include/LineExtractor.h:40-72, src/LineExtractor.cc:31-67) ------------------ */
/* per-image capacity of the key line / LBD descriptor records (lsd_nfeatures, or the detector's own
 * limit when lsd_nfeatures == 0) */
int olf_line_capacity(const olf_ctx* ctx);
/* Lineextractor::operator()(image, mask [ignored], keylines, descriptors_line): LSDDetectorC::detect with
 * the context's LSD options, top-N by response, BinaryDescriptor::compute (LBD). */
int olf_line_extract_strided(olf_ctx* ctx, const uint8_t* image, size_t row_stride, olf_keyline* kls, uint8_t* ldesc, int32_t* lcount);
int olf_line_extract_dev(olf_ctx* ctx, const uint8_t* d_images, int n_images, olf_keyline* d_kls, uint8_t* d_ldesc, int32_t* d_lcounts,
                         void* stream);
int olf_line_extract(olf_ctx* ctx, const uint8_t* images, int n_images, olf_keyline* kls, uint8_t* ldesc, int32_t* lcounts);
/* BinaryDescriptor::compute(image, keylines, descriptors) on caller-supplied key lines (host buffers;
 * Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:524-687): kls [n_images][capacity], counts[n_images].
 * Only sPointInOctaveX/Y, ePointInOctaveX/Y, numOfPixels and angle of a key line are read.  Accepted domain: the four coordinates
 * finite and within +-1e6, the angle finite, numOfPixels any int32 (the reference casts it to short: a value that casts to <= 0 gives
 * an all-zero descriptor).  Inside that domain the key lines may lie anywhere, outside the image included: sample coordinates beyond
 * +-32767 wrap through the reference's (short) cast (modulo 65536, as its x86 build does) before they are clamped into the image.
 * With conv_libm_float = 1 the angle must also satisfy |angle| < 120: the device's cosf / sinf restate glibc's fast range reduction
 * only, which is what glibc itself uses below 120.  A key line inside its image's count that leaves the domain fails the call with
 * OLF_ERR_INVALID and a message, before anything is uploaded or launched; records past the count are not looked at. */
int olf_lbd_compute(olf_ctx* ctx, const uint8_t* images, int n_images, const olf_keyline* kls, const int32_t* lcounts, uint8_t* ldesc);
/* debug/test: the sigma-0.6 blurred, x1.2 upsampled LSD working image of `image` (dst >= ws*hs bytes) */
int olf_lsd_debug_scaled(olf_ctx* ctx, int image, uint8_t* dst, int32_t* ws, int32_t* hs);

/* ---- Frame::ComputeStereoMatches_Lines (src/Frame.cc:878-1000) + matchGrid (src/LineMatcher.cpp:220-299) */
/* key lines / LBD descriptors of images 2p (left) and 2p+1 (right), stride olf_line_capacity().
 * Outputs per pair, stride capacity: matches_12 (-1 = none), mvDisparity_l (2 floats, -1 = mono),
 * mvle_l (3 doubles, 0 = mono). */
int olf_stereo_lines_dev(olf_ctx* ctx, int n_pairs, const olf_keyline* d_kls, const uint8_t* d_ldesc, const int32_t* d_lcounts,
                         int32_t* d_matches12, float* d_disp, double* d_le, void* stream);
int olf_stereo_lines(olf_ctx* ctx, int n_pairs, const olf_keyline* kls, const uint8_t* ldesc, const int32_t* lcounts, int32_t* matches12,
                     float* disp, double* le);

/* ---- fused entry: the feature part of Frame::Frame (stereo + lines), src/Frame.cc:136-221 -------- */
typedef struct olf_frame_buffers {
    olf_keypoint* kps;      /* [2*n_pairs][orb capacity]      mvKeys / mvKeysRight                   */
    uint8_t*  desc;         /* [2*n_pairs][orb capacity][32]  mDescriptors / mDescriptorsRight       */
    int32_t*  counts;       /* [2*n_pairs]                    N, Nr                                  */
    float*    uright;       /* [n_pairs][orb capacity]        mvuRight                               */
    float*    depth;        /* [n_pairs][orb capacity]        mvDepth                                */
    olf_keyline* kls;       /* [2*n_pairs][line capacity]     mvKeys_Line / mvKeysRight_Line         */
    uint8_t*  ldesc;        /* [2*n_pairs][line capacity][32] mDescriptors_Line / mDescriptorsRight_Line */
    int32_t*  lcounts;      /* [2*n_pairs]                                                           */
    int32_t*  lmatches12;   /* [n_pairs][line capacity]       stereo line matches (left -> right)    */
    float*    ldisp;        /* [n_pairs][line capacity][2]    mvDisparity_l                          */
    double*   lle;          /* [n_pairs][line capacity][3]    mvle_l                                 */
} olf_frame_buffers;
/* ExtractORB x2 + ExtractLine x2 (the reference's 4 threads, src/Frame.cc:164-171, here two HIP streams),
 * ComputeStereoMatches, ComputeStereoMatches_Lines, for n_pairs stereo pairs.  All pointers in `out` are
 * device pointers for the _dev form, host pointers otherwise. */
int olf_stereo_frames_dev(olf_ctx* ctx, const uint8_t* d_images, int n_pairs, const olf_frame_buffers* out, void* stream);
int olf_stereo_frames(olf_ctx* ctx, const uint8_t* images, int n_pairs, const olf_frame_buffers* out);

/* ---- Frame::mGrid and Frame::GetFeaturesInArea on the device (layout: orbline_types.h, "Frame::mGrid as two arrays") --------------------
 * void Frame::AssignFeaturesToGrid() (src/Frame.cc:334-349, PosInGrid :572-582; called by Frame::Frame at :215) for n_frames frames: frame j is
 * image j * img_stride of the key point / count buffers of olf_orb_extract_dev / olf_stereo_frames_dev (stride olf_orb_capacity(); img_stride 2 =
 * the left images of a stereo batch -- the convention of olf_search_by_bow_batch_dev).  Called on the stream given to olf_stereo_frames_dev right
 * after that call it delivers the batch's mGrid: the point outputs are final on that stream, with or without the deferred join.  The bounds are
 * mnMinX .. mnMaxY; the caller passes undistorted key points (mvKeysUn) -- what the extractor returns for a rectified camera (src/Frame.cc:601-605).
 * wInv = 64.f / (maxX - minX) and hInv = 48.f / (maxY - minY) are formed once in float (:186-187); posX = round((x - minX) * wInv), C round() on the
 * float product; a feature is kept iff 0 <= posX < 64 && 0 <= posY < 48.  d_cell_offsets [n_frames][OLF_GRID_CELLS + 1]; d_cell_index
 * [n_frames][olf_orb_capacity()].  A count beyond the capacity is read as the capacity.  Contexts whose olf_orb_capacity() exceeds
 * OLF_GRID_MAX_KEYS are refused (OLF_ERR_CAPACITY); maxX <= minX or maxY <= minY is OLF_ERR_INVALID. */
int olf_frame_grid_dev(olf_ctx* ctx, int n_frames, int img_stride, const olf_keypoint* d_kps, const int32_t* d_counts, float minX, float maxX,
                       float minY, float maxY, int32_t* d_cell_offsets, int32_t* d_cell_index, void* stream);
/* host buffers, one frame of n <= OLF_GRID_MAX_KEYS key points (more: OLF_ERR_CAPACITY; n == 0 gives all-zero offsets): uploads, runs the same kernel,
 * downloads.  cell_offsets [OLF_GRID_CELLS + 1], cell_index [n]. */
int olf_frame_grid(olf_ctx* ctx, const olf_keypoint* keys, int n, float minX, float maxX, float minY, float maxY, int32_t* cell_offsets,
                   int32_t* cell_index);
/* vector<size_t> Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:517-570) for n_queries queries on one frame's key points and
 * grid: exactly the CSR olf_match_candidates_dev consumes -- d_cand_idx[d_cand_offsets[q] .. d_cand_offsets[q + 1]) is the reference's vIndices of query
 * q in the reference's order (ix outer, iy inner, stored order inside a cell).  d_cand_offsets [n_queries + 1] is always complete, so a caller can size
 * a retry; nothing is written at or past cand_capacity, and a total beyond it sets the context's capacity flag (olf_ctx_synchronize /
 * olf_ctx_poll_status, as for olf_frames_pack_dev). */
int olf_features_in_area_dev(olf_ctx* ctx, const olf_keypoint* d_keys, const int32_t* d_cell_offsets, const int32_t* d_cell_index, float minX, float maxX,
                             float minY, float maxY, int n_queries, const olf_area_query* d_queries, int32_t* d_cand_offsets, int32_t* d_cand_idx,
                             int cand_capacity, void* stream);
/* host buffers (n_keys key points; the grid is checked as the searches check a supplied one): OLF_ERR_CAPACITY when cand_capacity is too small --
 * cand_offsets is complete then and cand_idx holds the first cand_capacity entries. */
int olf_features_in_area(olf_ctx* ctx, const olf_keypoint* keys, int n_keys, const int32_t* cell_offsets, const int32_t* cell_index, float minX,
                         float maxX, float minY, float maxY, int n_queries, const olf_area_query* queries, int32_t* cand_offsets, int32_t* cand_idx,
                         int cand_capacity);
/* The context's own device arrays, which the host-pointer entry points stage through: after olf_stereo_frames / olf_stereo_points / olf_orb_extract they
 * hold that call's results (until the next host-pointer call), so a *_dev entry can go on from them without another upload. */
int olf_ctx_device_buffers(const olf_ctx* ctx, olf_frame_buffers* out);

/* getLineCoords(x1, y1, x2, y2, line_coords), src/gridStructure.cpp:33-41: cells of the reference's Bresenham walk (src/LineIterator.cpp), host
 * arithmetic.  xy receives up to cap (x, y) pairs, *n the number of cells. */
int olf_line_coords(double x1, double y1, double x2, double y2, int32_t* xy, int cap, int32_t* n);

/* ---- multi-GPU: the trimmed wire record of a batch ------------------------------------------------------------------
 * What a rank sends to rank 0 after a batch: header, counts, then only the rows in use of every array of olf_frame_buffers (layout in
 * csrc/records.hip; host mirror and parser in orb_line_slam_amd/records.py).  `out` holds device pointers; d_dst >= olf_frames_pack_bound
 * bytes is always enough; *d_bytes (device or pinned host memory) receives the record size.  A record larger than dst_capacity sets the
 * capacity flag (olf_ctx_synchronize) and writes only the header. */
size_t olf_frames_pack_bound(const olf_ctx* ctx, int n_pairs);
int olf_frames_pack_dev(olf_ctx* ctx, const olf_frame_buffers* out, int n_pairs, uint8_t* d_dst, size_t dst_capacity, uint64_t* d_bytes, void* stream);
/* The map points a frame owns right after stereo matching: d_mask[i] = d_depth[i] > 0, the test of Tracking::StereoInitialization /
 * UpdateLastFrame on mvDepth (src/Tracking.cc:584-588, 1096-1099: `float z = mvDepth[i]; if(z>0)`), as the byte mask d_mp_valid of
 * olf_search_by_bow_batch_dev.  n = number of floats (n_pairs * olf_orb_capacity() for the depth plane of olf_stereo_points_dev);
 * d_depth 16-byte aligned, d_mask 4-byte aligned. */
int olf_stereo_points_mask_dev(olf_ctx* ctx, const float* d_depth, size_t n, uint8_t* d_mask, void* stream);

/* ---- ORBmatcher::SearchByProjection(Frame&, const Frame&, ...) for a batch on the device (csrc/track_batch.hip) -------------------------------
 * The frames of a batch in the roles the search reads them in.  Device pointers; frame j = image j * img_stride of the extractor-layout arrays
 * (img_stride 2 = the left images of a stereo batch, as olf_search_by_bow_batch_dev / olf_frame_grid_dev); the per-frame planes are
 * [n_frames][olf_orb_capacity()].  desc / mp_desc 16-byte aligned. */
typedef struct olf_track_batch {
    const olf_keypoint* kps; const uint8_t* desc; const int32_t* counts; int32_t img_stride;   /* mvKeysUn, mDescriptors, N */
    const float*   uright;            /* mvuRight                         (olf_frame_buffers.uright)                 */
    const int32_t* cell_offsets;      /* [n_frames][OLF_GRID_CELLS + 1]   (olf_frame_grid_dev)                       */
    const int32_t* cell_index;        /* [n_frames][capacity]                                                        */
    const float*   Tcw;               /* [n_frames][16] mTcw, row-major                                              */
    const float*   mp_world;          /* [n_frames][capacity][3] pMP->GetWorldPos() of the frame in its LastFrame role (olf_unproject_stereo_dev) */
    const uint8_t* mp_valid;          /* mvpMapPoints[i] != NULL      NULL: every feature holds one (olf_stereo_points_mask_dev) */
    const uint8_t* mp_obs;            /* pMP->Observations() > 0      NULL: all do (key-frame points); temporal points of UpdateLastFrame: 0 */
    const uint8_t* outlier;           /* mvbOutlier                   NULL: none                                      */
    const uint8_t* mp_desc;           /* pMP->GetDescriptor() [n_frames][capacity][32]   NULL: the frame's own descriptors */
    float fx, fy, cx, cy, mbf, minX, maxX, minY, maxY;
} olf_track_batch;
/* int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono) (src/ORBmatcher.cc:1330-1472) and the
 * overload with map<int,int>& match12 (:1474-1618), the matcher of Tracking::TrackWithMotionModel[WithLine] (src/Tracking.cc:1296,1302), for the
 * n_frames - 1 pairs of consecutive frames of a batch: pair j has LastFrame = frame j and CurrentFrame = frame j + 1.  The CurrentFrame starts without
 * map points (both call sites fill(..., NULL) first, src/Tracking.cc:1295,1301); mvScaleFactors are the context's.  Arithmetic: that of
 * olf_search_by_projection (convention C.12).  d_th (or NULL) [n_frames - 1]: a radius per pair that replaces th; an entry <= 0 skips the pair and leaves
 * its three output rows untouched -- the wider retry of src/Tracking.cc:1299-1303 is a second call with d_th[j] = nmatches[j] < 20 ? 2 * th : 0.
 * d_matches [n_frames - 1][capacity]: the LastFrame index whose point CurrentFrame feature i2 holds at the end (-1: none; -1 from N on);
 * d_match12 (or NULL), same shape: the value the reference's map holds under key i2 (the FIRST index, :1577), -1: no such key; d_nmatches [n_frames - 1]:
 * the return values.  A LastFrame feature that reaches its window with an octave outside the context's levels (caller-made key points) makes its pair
 * end with nmatches = -1 and its rows untouched, and sets bit 256 of the context's status word (olf_ctx_synchronize / olf_ctx_poll_status report it).
 * There is no other limit: the lists the search keeps are bounded per query and a query that outgrows them is recomputed.  n_frames < 2: nothing is
 * written.  Contexts above OLF_GRID_MAX_KEYS: OLF_ERR_CAPACITY; maxX <= minX or maxY <= minY: OLF_ERR_INVALID. */
int olf_search_by_projection_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, float th, const float* d_th, int bMono,
                                       int check_orientation, int32_t* d_matches, int32_t* d_match12, int32_t* d_nmatches, void* stream);
/* cv::Mat Frame::UnprojectStereo(const int &i) (src/Frame.cc:1073-1087) for every feature of n_frames frames -- the world positions of the stereo
 * points a frame owns (Tracking::UpdateLastFrame, src/Tracking.cc:1096-1101), i.e. mp_world of olf_track_batch.  invfx = 1.0f / fx and invfy are formed
 * once in float (:188-189); x = (u - cx) * z * invfx left to right in float; world = mRwc * x3Dc + mOw under C.12.  d_depth [n_frames][capacity] (mvDepth),
 * d_Twc [n_frames][16]: camera to world, rows of mRwc | mOw; d_world [n_frames][capacity][3].  Features with z <= 0 (the reference returns an empty
 * cv::Mat) or past the count get (0, 0, 0); their validity is the byte of olf_stereo_points_mask_dev. */
int olf_unproject_stereo_dev(olf_ctx* ctx, int n_frames, int img_stride, const olf_keypoint* d_kps, const int32_t* d_counts, const float* d_depth,
                             float fx, float fy, float cx, float cy, const float* d_Twc, float* d_world, void* stream);

/* ---- Tracking::SearchLocalPoints for a batch on the device (csrc/local_batch.hip) ------------------------------------------------------------------
 * The point half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1877-1942): Frame::isInFrustum for every local map point, then
 * ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th).
 *
 * The map the frames of a batch are matched against, as arrays of n_mp points (device pointers), and optionally each frame's mvpLocalMapPoints as a
 * list of indices into them.  Entries: with list_offsets, entry e in [list_offsets[j], list_offsets[j + 1]) is the (e - list_offsets[j])-th local map
 * point of frame j, the point list_index[e] -- the reference's iteration order; list_offsets[n_frames] <= n_entries.  With list_offsets == NULL every
 * frame sees all n_mp points in index order: entry e = j * n_mp + i is point i for frame j, there are n_frames * n_mp entries, and list_index / n_entries
 * are not read.  Every per-entry array of the two calls below is indexed by e. */
typedef struct olf_local_map {
    const float*   world;         /* [n_mp][3] GetWorldPos()                                                                       */
    const float*   normal;        /* [n_mp][3] GetNormal()                                                                         */
    const float*   maxd;          /* [n_mp] mfMaxDistance, unscaled (GetMaxDistanceInvariance() / 1.2f), as olf_is_in_frustum      */
    const float*   mind;          /* [n_mp] mfMinDistance, unscaled                                                                */
    const uint8_t* desc;          /* [n_mp][32] GetDescriptor(), 16-byte aligned                                                   */
    const uint8_t* obs;           /* [n_mp] Observations() > 0                                                                     */
    const uint8_t* bad;           /* [n_mp] isBad()                                                                                */
    int32_t        n_mp;
    const int32_t* list_offsets;  /* [n_frames + 1], non-decreasing from >= 0, or NULL                                             */
    const int32_t* list_index;    /* [n_entries]                                                                                   */
    int32_t        n_entries;
} olf_local_map;
/* int MapPoint::PredictScale(const float &currentDist, Frame* pF) (src/MapPoint.cc:414-429) as a table.  Host only, no context.  thr[k - 1], for
 * k = 1 .. n_levels - 1, is the smallest positive float `ratio` (= mfMaxDistance / currentDist) at which the host searches' own evaluation of PredictScale
 * (csrc/predict_scale.hpp: ceil(logf(ratio) / logf(scale_factors[1])), clamped to [0, n_levels - 1]) returns >= k -- found by bisection over the float bit
 * patterns on that function, so the predicted level is the number of thresholds <= ratio and the device needs no logarithm.  That rests on the level not
 * decreasing with the ratio, which is a property of the libm in use: the call checks the 4096 floats on either side of every threshold and returns
 * OLF_ERR_INVALID if the level is not constant on each side (or if a level is never reached, or scale_factors[1] <= 1).  thr [n_levels - 1]; n_levels = 1
 * writes nothing. */
int olf_predict_scale_thresholds(const float* scale_factors, int n_levels, float* thr);
/* bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit) (src/Frame.cc:388-444) for every entry of every frame, with the two tests
 * Tracking::SearchLocalPointsAndLines makes first (src/Tracking.cc:1880-1896, :1921-1924).  Arithmetic: that of olf_is_in_frustum, operation for
 * operation; the level comes from olf_predict_scale_thresholds of the context's mvScaleFactors.  `in`: only Tcw, the calibration and the bounds are read --
 * and counts (with img_stride) when d_frame_mp is given and counts is not NULL: frame j then holds d_frame_mp[j][0 .. N).
 * d_frame_mp [n_frames][capacity] (or NULL: the frames hold nothing): mvpMapPoints on entry as indices into the map; negative = none, or a point outside
 * the map (a temporal point).  A held point that is bad is dropped from its feature first, as :1885-1888 does.
 * An entry is skipped (in view = 0) when its point is bad (:1923) or is held by a feature of its frame (mnLastFrameSeen == mCurrentFrame.mnId, :1921).
 * Outputs per entry: d_in_view (uint8, mbTrackInView), d_level (mnTrackScaleLevel), d_view_cos (mTrackViewCos), d_proj3 (mTrackProjX, mTrackProjY,
 * mTrackProjXR); an entry that is skipped or fails a gate only gets in view = 0, as with olf_is_in_frustum.  MapPoint::IncreaseVisible (:1891, :1928) is
 * the caller's, from d_frame_mp and d_in_view.  A list index outside [0, n_mp) is left out (in view = 0) and a d_frame_mp value >= n_mp counts as "holds
 * nothing"; either sets bit 512 of the context's status word (olf_ctx_synchronize / olf_ctx_poll_status).  Entries outside every frame's list get
 * in view = 0.  Scratch: one bit per (frame, map point). */
int olf_is_in_frustum_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp,
                                float viewing_cos_limit, uint8_t* d_in_view, int32_t* d_level, float* d_view_cos, float* d_proj3, void* stream);
/* The frustum pass above (into context scratch), then int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)
 * (src/ORBmatcher.cc:47-131) for every frame, F.mvpMapPoints being d_frame_mp without its bad points.  `in`: kps, desc, counts, img_stride, uright, the
 * grids of olf_frame_grid_dev, Tcw, the calibration and the bounds are read; mvScaleFactors are the context's.  d_th (or NULL) [n_frames]: a radius
 * factor per frame that replaces th (the reference uses 1, 3 and 5, src/Tracking.cc:1935-1940); an entry <= 0 skips the frame and leaves its rows
 * untouched.  bFactor is `th != 1.0` of the factor in force for the frame.  mfNNratio = nnratio and viewing_cos_limit (0.8 and 0.5 at this call site).
 * d_matches [n_frames][capacity]: the MAP index feature idx received in this call (-1: none; -1 from N on); d_nmatches [n_frames]: the return values --
 * they count events: a feature that receives a point without observations can receive another one later, and both count (as olf_search_local_map).
 * Results equal a loop of olf_is_in_frustum + olf_search_local_map over the frames.  There is no capacity to exceed: the search keeps 16 bytes per entry
 * and recomputes an entry that outgrows them.  Errors: contexts above OLF_GRID_MAX_KEYS: OLF_ERR_CAPACITY; maxX <= minX, maxY <= minY or a NULL
 * required pointer: OLF_ERR_INVALID.  Malformed indices as above (bit 512), never out of bounds.  n_frames == 0 writes nothing; no entries: the rows
 * are -1 / 0.  Scratch: 37 bytes per entry, one bit per (frame, map point) and per (frame, feature). */
int olf_search_local_map_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp,
                                   float viewing_cos_limit, float th, const float* d_th, float nnratio, int32_t* d_matches, int32_t* d_nmatches,
                                   void* stream);

/* ---- ORBmatcher::SearchForTriangulation for a list of key-frame pairs on the device (csrc/triangulation_batch.hip) ----------------------------------
 * int ORBmatcher::SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, cv::Mat F12, vector<pair<size_t,size_t>> &vMatchedPairs, const bool bOnlyStereo,
 * const cv::Mat Cw) (src/ORBmatcher.cc:659-825), the matcher of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:268), for n_pairs pairs of the
 * n_frames frames of a batch, Frame::ComputeBoW of every frame included: each frame's FeatureVector is built once per call, whatever the number of pairs
 * it is part of (voc, levelsup: as olf_search_by_bow_batch_dev; 4 in the reference).  Results equal olf_search_for_triangulation pair by pair.
 * `in`: only kps, desc, counts, img_stride, uright, Tcw, mp_valid and fx, fy, cx, cy are read (frame j = image j * img_stride).  mp_valid keeps its
 * meaning -- the features that hold a map point, which this search skips on both sides -- so NULL (every feature holds one) searches nothing: rows -1,
 * counts 0.  mvScaleFactors are the context's.  d_pairs [n_pairs][2] = (kf1, kf2) frame indices, any order, a frame in any number of pairs.
 * d_F12 [n_pairs][9] row-major, used as x1^T F12 x2 (LocalMapping::ComputeF12: olf_compute_f12_pairs_dev).  d_Cw [n_pairs][3] = pKF1->GetCameraCenter(), or NULL:
 * -Rcw.t() * tcw of kf1's Tcw.  d_matches12 [n_pairs][capacity]: row p holds per feature idx1 of kf1 the matched feature idx2 of kf2 or -1 (-1 from N1
 * on); vMatchedPairs is the list of (idx1, d_matches12[p][idx1] >= 0) in idx1 order.  d_nmatches [n_pairs]: the return values.
 * A pair whose index lies outside [0, n_frames), or with kf1 == kf2, ends with nmatches = -1 and its row untouched, and sets bit 2048 of the context's
 * status word (olf_ctx_synchronize / olf_ctx_poll_status report it).  So does, with bit 256, a pair in which a candidate of key frame 2 holds an octave
 * outside the context's levels.  A candidate here is a feature of kf2 without a map point that passes only_stereo and shares its vocabulary node with a
 * searched feature of kf1: the test is made for every one of them, whereas olf_search_for_triangulation makes it only for those within TH_LOW of a query,
 * so this entry can refuse a pair the host form accepts.  The other pairs of the call are unaffected by either.
 * n_pairs == 0 or n_frames == 0: nothing is written.  Contexts above 4096 features per frame: OLF_ERR_CAPACITY (16 index bits in the sort key of the
 * FeatureVector stage); a NULL required pointer or a negative count: OLF_ERR_INVALID, before any launch.  Scratch: 12 bytes per (frame, feature). */
int olf_search_for_triangulation_batch_dev(olf_ctx* ctx, const olf_voc* voc, const olf_track_batch* in, int n_frames, int n_pairs,
                                           const int32_t* d_pairs, const float* d_F12, const float* d_Cw, int only_stereo, int check_orientation,
                                           int levelsup, int32_t* d_matches12, int32_t* d_nmatches, void* stream);

/* ---- ORBmatcher::SearchByBoW for a list of key-frame pairs on the device, both overloads (csrc/bow_match.hip) ------------------------------------------
 * The matcher of Tracking::TrackReferenceKeyFrame (src/Tracking.cc:963-970), Tracking::Relocalization (:2240-2261: one frame against every candidate key
 * frame) and LoopClosing::ComputeSim3 (src/LoopClosing.cc:271: the current key frame against every loop candidate) for n_pairs pairs of the n_frames
 * frames of a batch, Frame::ComputeBoW (src/Frame.cc:585-597) of every frame included: each frame's FeatureVector is built once per call, whatever the
 * number of pairs it is part of (voc, levelsup: as olf_search_by_bow_batch_dev; 4 in the reference).
 * `in`: only kps (angles), desc, counts, img_stride and mp_valid are read, everything else may be NULL or zero (frame j = image j * img_stride; a count
 * beyond the capacity is read as the capacity).  mp_valid keeps its meaning, mvpMapPoints[i] != NULL (NULL: every feature holds one); d_mp_bad
 * [n_frames][capacity] is isBad() of the held point (NULL: none is bad).  d_pairs [n_pairs][2] = (first, second) frame indices, any order, duplicates
 * allowed, a frame in any number of pairs.
 * form OLF_BOW_KF_FRAME: SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBmatcher.cc:161-290), first = pKF, second = F.
 * F starts without matches (:165) and its own mp_valid / bad flags are not read; a key-frame feature is searched when it holds a point that is not bad
 * (:193-199); a feature of F that holds a match from this call is passed over (:211-212); accept iff bestDist1 <= TH_LOW and (float)bestDist1 <
 * nnratio * (float)bestDist2 (:230-232).  Row p of d_matches [n_pairs][capacity] is indexed by the feature of F and holds the key-frame feature whose
 * point it received (-1: none; -1 from N_F on).  With the pairs (j, j + 1) rows and counts equal olf_search_by_bow_batch_dev's.
 * form OLF_BOW_KF_KF: SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (:524-657).  A feature of pKF1 is searched when it
 * holds a good point (:558-564); a feature of pKF2 is a candidate when it holds a good point and is not yet in vbMatched2 (:578-582); accept iff
 * bestDist1 < TH_LOW (strict, :600) and the same ratio test.  Row p is indexed by idx1 and holds idx2 or -1 (-1 from N1 on); the rotation histogram
 * drops by idx1 (:640-652).  Results equal olf_search_by_bow_kf pair by pair.
 * Both: d_nmatches [n_pairs] = the return values after the rotation check (ComputeThreeMaxima, only with check_orientation); on equal distances the
 * earlier candidate of the reference's scan stays.  Results do not depend on scheduling.
 * A pair whose index lies outside [0, n_frames), or with first == second, ends with nmatches = -1 and its row untouched, and sets bit 2048 of the context's
 * status word (olf_ctx_synchronize / olf_ctx_poll_status report it), as in olf_search_for_triangulation_batch_dev; the other pairs are unaffected.
 * Errors, before any launch: a NULL required pointer, a negative count, an unknown form or an empty vocabulary: OLF_ERR_INVALID; contexts above 4096
 * features per frame: OLF_ERR_CAPACITY (16 index bits in the sort key of the FeatureVector stage).  n_pairs == 0 or n_frames == 0: nothing is written.
 * Scratch: 12 bytes per (frame, feature).  The call does not synchronise. */
#define OLF_BOW_KF_FRAME 0   /* SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches),  src/ORBmatcher.cc:161-290 */
#define OLF_BOW_KF_KF    1   /* SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12), src/ORBmatcher.cc:524-657 */
int olf_search_by_bow_pairs_dev(olf_ctx* ctx, const olf_voc* voc, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs,
                                const uint8_t* d_mp_bad, int form, float nnratio, int check_orientation, int levelsup,
                                int32_t* d_matches, int32_t* d_nmatches, void* stream);

/* ---- the search part of ORBmatcher::Fuse for a batch of key frames on the device (csrc/fuse_batch.hip) ------------------------------------------------
 * int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint*> &vpMapPoints, const float th) (src/ORBmatcher.cc:827-948), called per target key frame by
 * LocalMapping::SearchInNeighbors (src/LocalMapping.cc:454-534, calls at :489 and :514), and int ORBmatcher::Fuse(KeyFrame *pKF, cv::Mat Scw,
 * const vector<MapPoint*> &vpPoints, float th, vector<MapPoint*> &vpReplacePoint) (:977-1102), called per corrected key frame by
 * LoopClosing::SearchAndFuse (src/LoopClosing.cc:605): for every key frame of a batch and every point of its list the most similar key point inside the
 * projection window.  Results equal olf_fuse_search / olf_fuse_search_sim3 key frame by key frame; the map mutation that follows (:950-972, :1086-1099)
 * stays the caller's (INTEGRATION.md says when a result goes stale).
 * `in`: kps, desc, counts, img_stride, uright, the grids of olf_frame_grid_dev, Tcw, the calibration with mbf and the bounds are read (frame j = image
 * j * img_stride; a count beyond the capacity is read as the capacity); mvScaleFactors and the PredictScale thresholds are the context's.
 * `map`: the points and every key frame's list as entries, exactly as olf_search_local_map_batch_dev reads olf_local_map (list_offsets == NULL: every key
 * frame sees all n_mp points -- all target key frames against the current key frame's points, all corrected key frames against mvpLoopMapPoints);
 * world, normal, maxd, mind (unscaled), desc and bad are read, obs is not.
 * d_frame_mp [n_frames][capacity] (or NULL: the key frames hold nothing): mvpMapPoints as indices into the map, negative = none.  An entry whose point the
 * key frame holds is skipped: pMP->IsInKeyFrame(pKF) (:851) in the plain form, spAlreadyFound.count(pMP) with spAlreadyFound = pKF->GetMapPoints() (:992,
 * :1007) in the Sim3 form; so is a bad point, in both.
 * d_Scw: NULL gives the plain form -- the pose is in->Tcw, the stereo / mono chi-square gate is on, "nothing" is -1 / 256; [n_frames][16] (row-major)
 * gives the Sim3 form -- the pose is decomposed as :985-989 does, there is no chi-square gate, "nothing" is -1 / INT_MAX, in->Tcw is not read.
 * d_Ow [n_frames][3] = pKF->GetCameraCenter(), or NULL: -Rcw.t() * tcw of Tcw; plain form only, the Sim3 form ignores it.
 * d_best_idx / d_best_dist: per entry, indexed like every per-entry array of olf_local_map; entries outside every list get the "nothing" pair.
 * d_nfused [n_frames] (or NULL): the number of the frame's entries with best_idx >= 0 && best_dist <= TH_LOW (50) -- what Fuse would return before any
 * map mutation; 0 without entries.
 * Errors, before any launch: a NULL required pointer, a negative count, maxX <= minX or maxY <= minY: OLF_ERR_INVALID; contexts above OLF_GRID_MAX_KEYS:
 * OLF_ERR_CAPACITY.  A list index or a d_frame_mp value outside the map is left out and sets bit 512 of the context's status word (olf_ctx_synchronize /
 * olf_ctx_poll_status), as in olf_search_local_map_batch_dev.  In the plain form a candidate that passes the level gate with an octave outside the
 * context's levels -- that can only be octave -1 under predicted level 0 -- is left out of its window and sets bit 256; every other candidate and entry is
 * unaffected.  olf_fuse_search refuses the whole call there (OLF_ERR_INVALID): this entry answers for the rest of the batch.  n_frames == 0 writes nothing.
 * Scratch: 16 bytes per entry, 64 bytes per key frame and, with d_frame_mp, one bit per (frame, map point). */
int olf_fuse_search_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const olf_local_map* map, const int32_t* d_frame_mp,
                              const float* d_Scw, const float* d_Ow, float th, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_nfused,
                              void* stream);

/* ---- ORBmatcher::SearchBySim3 for a list of key-frame pairs on the device (csrc/sim3_batch.hip) ---------------------------------------------------------
 * int ORBmatcher::SearchBySim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12, const float &s12, const cv::Mat &R12, const cv::Mat &t12,
 * const float th) (src/ORBmatcher.cc:1104-1328), called per loop candidate by LoopClosing::ComputeSim3 (src/LoopClosing.cc:329) on the candidate's own
 * copy of the matches (:319): n_pairs pairs of the n_frames key frames of a batch, each with its own similarity.  Results equal olf_search_by_sim3 pair by
 * pair and do not depend on scheduling; INTEGRATION.md says why the candidates of one round are independent and when a row goes stale.
 * `in`: kps, desc, counts, img_stride, the grids of olf_frame_grid_dev, Tcw, mp_world, mp_valid (NULL: every feature holds a point), mp_desc (NULL: the
 * frame's own descriptors), fx, fy, cx, cy and the bounds are read (frame j = image j * img_stride; a count beyond the capacity is read as the capacity);
 * mvScaleFactors and the PredictScale thresholds are the context's.
 * d_mp_bad (or NULL: none is bad), d_mp_maxd, d_mp_mind [n_frames][capacity]: isBad(), mfMaxDistance and mfMinDistance of the point a feature holds, per
 * feature like mp_world; the distances unscaled as in olf_local_map -- the search applies 1.2 and 0.8 (GetMaxDistanceInvariance, :1179-1180).
 * d_pairs [n_pairs][2] = (kf1, kf2) frame indices, any order, duplicates allowed, a frame in any number of pairs and on either side.  d_s12 [n_pairs],
 * d_R12 [n_pairs][9] row-major, d_t12 [n_pairs][3]: the similarity of each pair, as the Sim3Solver hands it over (:325-327).
 * d_matches12 [n_pairs][capacity], in / out, the codes of olf_search_by_sim3: in -- -1 = NULL, >= 0 = pMP->GetIndexInKeyFrame(pKF2), -2 = a point pKF2
 * does not observe; a value >= N2 marks feature i1 as matched and nothing in kf2 (:1141) and never indexes anything; out -- additionally the agreed
 * matches.  Positions from N1 on are left as they are.
 * d_vn_match1, d_vn_match2 [n_pairs][capacity] (either may be NULL: the row then lives in context scratch): vnMatch1 / vnMatch2, -1 from N on.
 * d_nfound [n_pairs]: the return values.
 * A pair whose index lies outside [0, n_frames), or with kf1 == kf2, ends with nfound = -1 and its three rows untouched, and sets bit 2048 of the context's
 * status word (olf_ctx_synchronize / olf_ctx_poll_status report it), as in olf_search_for_triangulation_batch_dev and olf_search_by_bow_pairs_dev; the other
 * pairs are unaffected.  A window candidate that passes the level gate with an octave outside the context's levels -- that can only be octave -1 under
 * predicted level 0 -- is left out of its window and sets bit 256, as in olf_fuse_search_batch_dev (olf_search_by_sim3 takes it).
 * Errors, before any launch: a NULL required pointer (the per-pair arrays only when n_pairs > 0), a negative count, maxX <= minX or maxY <= minY:
 * OLF_ERR_INVALID; contexts above OLF_GRID_MAX_KEYS (or 2 * n_pairs * capacity beyond 2^31): OLF_ERR_CAPACITY.  n_pairs == 0 or n_frames == 0 writes
 * nothing.  The call does not synchronise.
 * Scratch: 128 bytes and one bit per feature of the capacity per pair, 12 bytes per (pair, direction, feature), and 4 bytes per (pair, feature) for each
 * of d_vn_match1 / d_vn_match2 that is NULL. */
int olf_search_by_sim3_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, const float* d_mp_maxd,
                                 const float* d_mp_mind, int n_pairs, const int32_t* d_pairs, const float* d_s12, const float* d_R12, const float* d_t12,
                                 float th, int32_t* d_matches12, int32_t* d_vn_match1, int32_t* d_vn_match2, int32_t* d_nfound, void* stream);

/* ---- the two key-frame forms of ORBmatcher::SearchByProjection for batches on the device (csrc/projection_batch.hip) ------------------------------------
 * Both are ordered greedy searches -- a key point that takes a point is closed to every later point -- solved as olf_search_by_projection_batch_dev and
 * olf_search_local_map_batch_dev solve theirs: at most 4 best candidates are kept per query, one wave walks the queries in the reference's order, and a
 * query that runs out of kept candidates is recomputed on the spot.  There is no capacity to exceed, and results do not depend on scheduling.
 *
 * int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, const float th, const int ORBdist)
 * (src/ORBmatcher.cc:1620-1747), called up to twice per candidate key frame by Tracking::Relocalization (src/Tracking.cc:2322, :2336) on the candidate's
 * own copy of the frame's map points and its own PnP pose: n_pairs pairs of the n_frames frames of a batch.  Rows and counts equal
 * olf_search_by_projection_kf pair by pair; INTEGRATION.md says why the candidates of one round are independent, how the second call is formed from the
 * first one's row and when a row goes stale.
 * `in`: kps, desc, counts, img_stride, the grids of olf_frame_grid_dev (of the current frames), fx, fy, cx, cy and the bounds are read; mp_world, mp_valid
 * (NULL: every feature holds a point) and mp_desc (NULL: the frame's own descriptors) in the key-frame role; Tcw only when d_Tcw is NULL; uright is not
 * read (the reference has no mvuRight gate here).  Frame j = image j * img_stride; a count beyond the capacity is read as the capacity.  mvScaleFactors
 * and the PredictScale thresholds are the context's.
 * d_mp_bad (or NULL: none is bad), d_mp_maxd, d_mp_mind [n_frames][capacity]: as olf_search_by_sim3_pairs_dev (unscaled; the search applies 1.2 and 0.8,
 * :1667-1668).  d_pairs [n_pairs][2] = (current frame, key frame), any order, duplicates allowed, a frame in any number of pairs and in either role.
 * d_Tcw [n_pairs][16] (or NULL: in->Tcw of the current frame): the pose of the current frame under this candidate, row-major.
 * d_cur_valid [n_pairs][capacity] (or NULL: none): CurrentFrame.mvpMapPoints[i2] != NULL on entry, per candidate -- such a feature is passed over (:1693).
 * d_already_found [n_pairs][capacity] (or NULL: none): sAlreadyFound.count(pKF's i-th point), indexed by the key-frame feature (:1648).
 * d_th [n_pairs] / d_orb_dist [n_pairs] (or NULL) replace th / orb_dist per pair; d_th[p] <= 0 skips the pair and leaves its row and count untouched.
 * Arithmetic: x3Dc = Rcw * x3Dw + tcw under C.12 and invzc = (float)(1.0 / z) with NO sign test -- the reference has none, so a point behind the camera
 * that lands inside the image is searched --, the CLOSED image bounds, dist3D from a double sum, the CLOSED interval [0.8f * mind, 1.2f * maxd], the
 * window over the levels nPredictedLevel - 1 .. nPredictedLevel + 1 with radius th * mvScaleFactors[nPredictedLevel], the best distance with `<` in
 * scan order, accepted iff <= orb_dist (a distance of 256 never registers), then with check_orientation the rotation histogram (ComputeThreeMaxima).
 * d_matches [n_pairs][capacity]: row p is indexed by the current frame's feature and holds the key-frame feature whose point it received in this call,
 * after the rotation check (-1: none; -1 from N on).  d_nmatches [n_pairs]: the return values.  The inputs are not written.
 * A pair whose index lies outside [0, n_frames), or with both indices equal, ends with nmatches = -1 and its row untouched, and sets bit 2048 of the
 * context's status word (olf_ctx_synchronize / olf_ctx_poll_status report it), as in the other pair entries; the other pairs are unaffected.
 * Errors, before any launch: a NULL required pointer (the per-pair arrays only when n_pairs > 0), a negative count, img_stride < 1, maxX <= minX or
 * maxY <= minY: OLF_ERR_INVALID; contexts above OLF_GRID_MAX_KEYS (or n_pairs * capacity beyond 2^31): OLF_ERR_CAPACITY.  n_pairs == 0 or
 * n_frames == 0 writes nothing.  The call does not synchronise.  Scratch: 32 bytes per (pair, feature). */
int olf_search_by_projection_kf_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, const float* d_mp_maxd,
                                          const float* d_mp_mind, int n_pairs, const int32_t* d_pairs, const float* d_Tcw, const uint8_t* d_cur_valid,
                                          const uint8_t* d_already_found, float th, const float* d_th, int orb_dist, const int32_t* d_orb_dist,
                                          int check_orientation, int32_t* d_matches, int32_t* d_nmatches, void* stream);
/* int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints, vector<MapPoint*> &vpMatched, int th)
 * (src/ORBmatcher.cc:292-405), called by LoopClosing::ComputeSim3 (src/LoopClosing.cc:381), for every key frame of a batch against its list of points.
 * Rows and counts equal olf_search_by_projection_sim3 key frame by key frame.
 * `in`: kps, desc, counts, img_stride, the grids of olf_frame_grid_dev, the calibration with mbf and the bounds are read; Tcw and uright are not.
 * `map`: the points and every key frame's list as entries, exactly as olf_fuse_search_batch_dev reads olf_local_map (list_offsets == NULL: every key
 * frame sees all n_mp points in index order); world, normal, maxd, mind (unscaled), desc and bad are read, obs is not.
 * d_Scw [n_frames][16] row-major: the Sim3 pose of each key frame, decomposed as :301-305 does.
 * d_frame_matched [n_frames][capacity], in / out: vpMatched as map indices.  In: -1 = NULL; >= 0 = the map index held -- that key point is closed (:378)
 * and that point is in spAlreadyFound (:307-308, :321); -2 (any other negative value) = a point outside the map -- that key point is closed only.  Out:
 * additionally the map index each key point received in this call; nothing else is written, positions from N on are left as they are.
 * d_th [n_frames] (or NULL) replaces th per key frame; an entry <= 0 skips the key frame and leaves its row and count untouched.  The reference's th is
 * an int (10 at the call site); the radius is th * mvScaleFactors[nPredictedLevel] in float.
 * Gates: those of olf_search_by_projection_sim3 -- the point gate of the Sim3 Fuse without a chi-square gate (depth, the HALF-OPEN image bounds, the
 * distance interval, the 60 degree gate), the predicted level from the thresholds, the unrestricted window, the level gate per candidate
 * (nPredictedLevel - 1 <= octave <= nPredictedLevel), the best distance with `<` in scan order, taken at once iff <= TH_LOW (50).  A candidate with
 * octave -1 under predicted level 0 passes the level gate as in the host form; no status bit is set.
 * d_nmatches [n_frames]: the return values (0 without entries).
 * A list index or a d_frame_matched value >= n_mp is left out -- the value still closes its key point -- and sets bit 512 of the context's status word, as
 * in olf_fuse_search_batch_dev.  Errors follow that entry: a NULL required pointer, a negative count, maxX <= minX or maxY <= minY: OLF_ERR_INVALID;
 * contexts above OLF_GRID_MAX_KEYS (or 2^31 entries): OLF_ERR_CAPACITY; before any launch.  n_frames == 0 writes nothing.  The call does not synchronise.
 * Scratch: 32 bytes per entry, 64 bytes per key frame and one bit per (key frame, map point). */
int olf_search_by_projection_sim3_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const olf_local_map* map, const float* d_Scw,
                                            int32_t* d_frame_matched, float th, const float* d_th, int32_t* d_nmatches, void* stream);

/* ---- the line half of tracking: Frame::isInFrustum_l, SearchLocalPointsAndLines' line half, the f2f line tracking (csrc/line_batch.hip) --------------------
 * Host forms first (host arithmetic, no device work, no context): they are the definition the device entries below equal, bit for bit.
 *
 * bool Frame::isInFrustum_l(MapLine *pML, float viewingCosLimit), src/Frame.cc:446-515, for n_ml map lines.  world6 [n_ml][6]: GetWorldPos(), start point
 * then end point, as float (Converter::toCvMat).  Per end point, the start point first: mRcw * p + mtcw (C.12), PcZ < 0 fails, invz = 1.0f / PcZ,
 * u = fx * PcX * invz + cx, the CLOSED image bounds -- the first half of olf_is_in_frustum.  f supplies mTcw, the calibration and the bounds.  Outputs per
 * line: in_view (mbTrackInView) and proj4 = (mTrackProjsX, mTrackProjsY, mTrackProjeX, mTrackProjeY); a line that fails only gets in_view = 0.
 * mnTrackangle (:512) is read by commented-out code only (src/Tracking.cc:1991-1997) and is not produced. */
int olf_is_in_frustum_l(const olf_frame_view* f, int n_ml, const float* world6, uint8_t* in_view, float* proj4);
/* The loop of Tracking::SearchLocalPointsAndLines over matches_12 (src/Tracking.cc:1974-2016) and n_inliers_ls (:2021-2023) for one frame.  The first four
 * arrays run over mvpLocalMapLines_InFrustum (n_in_view lines, the reference's i1): m12 (in / out: matches_12 of match(), :1970; the loop sets entries
 * to -1, :2010), map_index (the line's index into the map of n_ml lines), proj4 (of olf_is_in_frustum_l).  kls = mvKeysUn_Line, ldisp [n_lines][2] =
 * mvDisparity_l, frame_ml [n_lines] (in / out) = mvpMapLines as map indices, negative = NULL, on entry without its bad lines (:1897-1913); obs [n_ml] =
 * Observations() > 0.  deltaWidth = (double)(maxX - minX) * 0.1 with the subtraction in float; the coordinate differences are formed in float, widened
 * and compared with a strict '>'.  *n_inliers = n_inliers_ls.  An index outside its array is OLF_ERR_INVALID. */
int olf_local_lines_assign(int n_in_view, int32_t* m12, const int32_t* map_index, const float* proj4, const olf_keyline* kls, int n_lines, const float* ldisp,
                           float minX, float maxX, float minY, float maxY, int n_ml, const uint8_t* obs, int32_t* frame_ml, int32_t* n_inliers);
/* The f2f line tracking behind match(desc_last, desc_cur, nnr, matches_12) for one pair: Tracking::TrackWithMotionModelWithLine, src/Tracking.cc:1305-1349
 * (skip_null = 1: a last line that holds nothing is passed over, :1316; gates = 1, delta_angle = M_PI / 8.0, pos_frac = 0.1) and
 * TrackReferenceKeyFrameWithLine, :976-1020 (skip_null = 0: it is assigned as NULL and counted, :1018-1019; gates = 0: `if(false)`, :993).  m12 [n_last]
 * (in / out; the gates set entries to -1), last_ml [n_last]: the last frame's (key frame's) mvpMapLines as ids, negative = NULL; cur_ml [n_cur] (out):
 * filled with -1 (:1306, :977), then the ids assigned -- i1 runs upwards, the last assignment stays; *n_inliers counts assignments (:1348).  The angle
 * gate: the float difference of the angles, widened, +- 2 * M_PI in double, fabs(theta) > delta_angle; the position gate as above with pos_frac. */
int olf_track_lines_assign(int n_last, int32_t* m12, const olf_keyline* kls_last, const int32_t* last_ml, int n_cur, const olf_keyline* kls_cur,
                           const float* ldisp_cur, float minX, float maxX, float minY, float maxY, int skip_null, int gates, double delta_angle, double pos_frac,
                           int32_t* cur_ml, int32_t* n_inliers);

/* The frames of a batch in the role the line searches read them in.  Device pointers; frame j = image j * img_stride of the extractor-layout arrays
 * (img_stride 2 = the left images of a stereo batch); the per-frame planes are [n_frames][olf_line_capacity()].  ldesc 16-byte aligned. */
typedef struct olf_line_batch {
    const olf_keyline* kls; const uint8_t* ldesc; const int32_t* lcounts; int32_t img_stride;   /* mvKeysUn_Line (the caller's responsibility, as kps is), mDescriptors_Line, N_l */
    const float*   ldisp;             /* [n_frames][capacity][2] mvDisparity_l            (olf_frame_buffers.ldisp)                  */
    const float*   Tcw;               /* [n_frames][16] mTcw, row-major                                                              */
    float fx, fy, cx, cy, minX, maxX, minY, maxY;
} olf_line_batch;
/* The map lines the frames of a batch are matched against, as arrays of n_ml lines (device pointers), and optionally each frame's mvpLocalMapLines as a
 * list of indices into them: list_offsets / list_index / n_entries have the semantics of olf_local_map, and a NULL list_offsets means every frame sees
 * all lines in index order.  A line a frame holds must be one of the n_ml lines; it need not be in the frame's list. */
typedef struct olf_local_line_map {
    const float*   world;         /* [n_ml][6] GetWorldPos(): start, then end                                                      */
    const uint8_t* desc;          /* [n_ml][32] GetDescriptor(), 16-byte aligned                                                   */
    const uint8_t* obs;           /* [n_ml] Observations() > 0                                                                     */
    const uint8_t* bad;           /* [n_ml] isBad()                                                                                */
    int32_t        n_ml;
    const int32_t* list_offsets;  /* [n_frames + 1], non-decreasing from >= 0, or NULL                                             */
    const int32_t* list_index;    /* [n_entries]                                                                                   */
    int32_t        n_entries;
} olf_local_line_map;
/* Frame::isInFrustum_l (src/Frame.cc:446-515) for every entry of every frame, with the two skips Tracking::SearchLocalPointsAndLines makes first
 * (src/Tracking.cc:1953-1956): the line is held by the frame (mnLastFrameSeen == mCurrentFrame.mnId) or is bad.  Arithmetic: that of olf_is_in_frustum_l.
 * `in`: Tcw, the calibration and the bounds are read -- and lcounts (with img_stride) when d_frame_ml is given and lcounts is not NULL.
 * d_frame_ml [n_frames][capacity] (or NULL: the frames hold nothing): mvpMapLines on entry as indices into the map, negative = none.  A held line that is
 * bad is dropped first (:1902-1905).  Outputs per entry: d_in_view (uint8) and d_proj4 (4 floats, 16-byte aligned); an entry that is skipped or fails only
 * gets in view = 0.  MapLine::IncreaseVisible (:1908, :1961) is the caller's.  A list index outside [0, n_ml) is left out (in view = 0) and a d_frame_ml
 * value >= n_ml counts as "holds nothing"; either sets bit 1024 of the context's status word (olf_ctx_synchronize / olf_ctx_poll_status).  Accesses are never
 * out of bounds.  Uses the batch scratch slot (one bit per (frame, map line) when d_frame_ml is given, nothing otherwise) and does not synchronise, as the point entries.  Contexts whose olf_line_capacity() exceeds 4096:
 * OLF_ERR_CAPACITY; maxX <= minX, maxY <= minY or a NULL required pointer: OLF_ERR_INVALID; n_frames == 0 writes nothing. */
int olf_is_in_frustum_l_batch_dev(olf_ctx* ctx, const olf_line_batch* in, int n_frames, const olf_local_line_map* map, const int32_t* d_frame_ml,
                                  uint8_t* d_in_view, float* d_proj4, void* stream);
/* The line half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1897-1913, :1945-2023) for every frame: the pass above; the in-view lines of a frame
 * in list order are mvpLocalMapLines_InFrustum (:1963); match(mvpLocalMapLines_InFrustum, mCurrentFrame, nnr, matches_12) (:1970), which is matchNNR only
 * (src/LineMatcher.cpp:64-73): kNN(2) of the in-view map line descriptors against the frame's own, the ratio test d0 < d1 * nnr, a frame with fewer than
 * two lines matches nothing; the loop :1976-2016; n_inliers_ls (:2021-2023).  nnr = Config::minRatio12L().  Outputs per entry: d_in_view, d_proj4 as
 * above, d_m12: the value matches_12 holds at the end for the entry's place in mvpLocalMapLines_InFrustum, -1 for entries not in view.  Per frame:
 * d_frame_ml_out [n_frames][capacity]: mvpMapLines at the end as map indices (lines held on entry stay, bad ones are gone; -1 from N_l on; may be
 * d_frame_ml itself); d_ninliers [n_frames].  Results equal a loop of olf_is_in_frustum_l, olf_match_bf and olf_local_lines_assign over the frames and do
 * not depend on scheduling.  Errors and malformed indices as above.  Scratch: 17 bytes per entry, 8 per (frame, line), one bit per (frame, map line) when d_frame_ml is given. */
int olf_search_local_lines_batch_dev(olf_ctx* ctx, const olf_line_batch* in, int n_frames, const olf_local_line_map* map, const int32_t* d_frame_ml, float nnr,
                                     uint8_t* d_in_view, float* d_proj4, int32_t* d_m12, int32_t* d_frame_ml_out, int32_t* d_ninliers, void* stream);
/* The f2f line tracking of Tracking::TrackWithMotionModelWithLine (src/Tracking.cc:1305-1349) / TrackReferenceKeyFrameWithLine (:976-1020) for the
 * n_frames - 1 pairs of consecutive frames of a batch: pair j has last = frame j and current = frame j + 1.  match(desc_last, desc_cur, nnr, matches_12)
 * with best_lr = Config::bestLRMatches() (the kNN of olf_match_bf_dev), then olf_track_lines_assign's loop with the same flags and parameters.
 * d_last_ml [n_frames - 1][capacity]: mvpMapLines of pair j's last frame as ids, negative = NULL.  d_enable (or NULL) [n_frames - 1]: 0 leaves the pair's
 * three output rows untouched.  Outputs per pair: d_m12 [capacity] (-1 from the last frame's N_l on), d_cur_ml [capacity] (the ids copied from
 * d_last_ml, -1 = NULL), d_ninliers.  n_frames < 2: nothing is written.  Errors as above. */
int olf_track_lines_batch_dev(olf_ctx* ctx, const olf_line_batch* in, int n_frames, const int32_t* d_last_ml, float nnr, int best_lr, int skip_null, int gates,
                              double delta_angle, double pos_frac, const int32_t* d_enable, int32_t* d_m12, int32_t* d_cur_ml, int32_t* d_ninliers, void* stream);

/* ---- Tracking::UpdateLocalMap for a batch of frames on the device (csrc/localmap_batch.hip) -----------------------------------------------------------
 * void Tracking::UpdateLocalMap() (src/Tracking.cc:2028-2205) = UpdateLocalKeyFrames (:2080-2205), then UpdateLocalPointsAndLines (:2039-2078), for n_frames
 * frames against one snapshot of the map (olf_map_graph, orbline_types.h; device pointers here).  It produces what the two local searches start from:
 * d_mp_offsets / d_mp_index are list_offsets / list_index of the olf_local_map of olf_search_local_map_batch_dev, d_ml_offsets / d_ml_index those of the
 * olf_local_line_map of olf_search_local_lines_batch_dev, in the reference's order, element for element, under convention C.16: ascending
 * key-frame index stands for the iteration order of std::map<KeyFrame*,int> (:2083) and std::set<KeyFrame*> (GetChilds, :2172).  So the reference key frame
 * among equal vote counts is the lowest index, and the first list is in ascending index.
 * Frame j is image j * img_stride of d_counts / d_lcounts (N and N_l; NULL: every frame holds olf_orb_capacity() / olf_line_capacity() features);
 * d_frame_mp [n_frames][olf_orb_capacity()] and d_frame_ml [n_frames][olf_line_capacity()] (or NULL: the frames hold no lines) are mvpMapPoints /
 * mvpMapLines as map indices with the meaning they have for olf_search_local_map_batch_dev: negative = none, or a temporal point -- such a feature neither
 * votes nor is cleared.  A held point or line that is bad is cleared (:2097, :2114); lines do not vote (:2110).  d_frame_mp_out / d_frame_ml_out (NULL: not
 * wanted; may be the inputs themselves): the rows with the bad ones cleared to -1, -1 from N on, everything else as it came.
 * d_n_voted [n_frames]: the size of keyframeCounter, bad key frames included.  d_ref_kf [n_frames]: pKFmax, the first key frame in ascending index that is
 * not bad and has the most votes among those, -1 when there is none.  A frame with d_n_voted[j] == 0 gets d_ref_kf[j] = -1 and three empty lists: the
 * reference returns at :2120 and so keeps the previous frame's lists and reference key frame -- that chain across frames stays the caller's.  A frame whose
 * voted key frames are all bad gets an empty key-frame list (hence empty point and line lists) and d_ref_kf = -1.
 * d_kf_offsets [n_frames + 1] / d_kf_index [kf_capacity]: mvpLocalKeyFrames as a CSR; the extension loop (:2149-2198) visits the first list only (its end
 * iterator is taken before the loop), stops once the list holds more than 80, reads the first 10 covisible key frames, the children in ascending index and
 * the parent, which is not tested for isBad() and whose insertion ends the loop (:2194).  The three offset arrays are always complete, so a caller can size a
 * retry; nothing is written at or past a capacity, and a total beyond one sets bit 8192 of the context's status word (olf_ctx_synchronize /
 * olf_ctx_poll_status, as for olf_features_in_area_dev).
 * Malformed indices are left out, never dereferenced: a point index outside the map (d_frame_mp, kf_mp_index) sets status bit 512, a line index outside
 * the map bit 1024, a key-frame index outside [0, n_kf) (mp_obs_kf, kf_covis_index, kf_child_index, kf_parent other than -1) bit 4096.  Rows of a CSR are
 * clamped to [0, offsets[n]].  That every row of kf_child_index ascends strictly is the caller's contract here (olf_update_local_map checks it).
 * Errors: n_kf > OLF_LOCALMAP_MAX_KF (a frame's vote table lives in LDS): OLF_ERR_CAPACITY before anything is launched; a NULL required pointer or a negative
 * size: OLF_ERR_INVALID.  n_frames == 0 writes nothing.  Does not synchronise; runs on `stream` and uses the batch scratch slot: 4 bytes per (frame, key
 * frame) for the key-frame lists between its passes, and one bit per (frame, map point) and per (frame, map line) when the map holds more than 262144
 * points and lines together (up to there a frame's two bitmaps live in LDS). */
#define OLF_LOCALMAP_MAX_KF 8192
int olf_update_local_map_batch_dev(olf_ctx* ctx, const olf_map_graph* g, int n_frames, int img_stride, const int32_t* d_counts, const int32_t* d_lcounts,
                                   const int32_t* d_frame_mp, const int32_t* d_frame_ml, int32_t* d_frame_mp_out, int32_t* d_frame_ml_out, int32_t* d_ref_kf,
                                   int32_t* d_n_voted, int32_t* d_kf_offsets, int32_t* d_kf_index, int kf_capacity, int32_t* d_mp_offsets, int32_t* d_mp_index,
                                   int mp_capacity, int32_t* d_ml_offsets, int32_t* d_ml_index, int ml_capacity, void* stream);
/* host buffers, the graph's arrays included: checks the graph (offsets non-decreasing from 0; a row of kf_child_index that is not strictly ascending:
 * OLF_ERR_INVALID), uploads, runs the same kernels on the context's stream, downloads.  OLF_ERR_CAPACITY when a capacity is too small: the three offset
 * arrays are complete then and each index array holds its first `capacity` entries; the same code, with the message of the bit, for a malformed index. */
int olf_update_local_map(olf_ctx* ctx, const olf_map_graph* g, int n_frames, int img_stride, const int32_t* counts, const int32_t* lcounts,
                         const int32_t* frame_mp, const int32_t* frame_ml, int32_t* frame_mp_out, int32_t* frame_ml_out, int32_t* ref_kf, int32_t* n_voted,
                         int32_t* kf_offsets, int32_t* kf_index, int kf_capacity, int32_t* mp_offsets, int32_t* mp_index, int mp_capacity, int32_t* ml_offsets,
                         int32_t* ml_index, int ml_capacity);

/* ---- KeyFrame::UpdateConnections for a list of key frames on the device (csrc/connections_batch.hip) --------------------------------------------------
 * void KeyFrame::UpdateConnections() (src/KeyFrame.cc:446-557) for n_list key frames against one snapshot of the map (olf_map_graph, device pointers here):
 * the call of LocalMapping for every new key frame (src/LocalMapping.cc:164) and after SearchInNeighbors (:533), of Tracking for the two initial key frames
 * (src/Tracking.cc:822-823) and of LoopClosing::CorrectLoop over whole neighbourhoods (src/LoopClosing.cc:438, 521, 560).  It produces kf_covis_offsets /
 * kf_covis_index of an olf_map_graph on the device, which olf_update_local_map_batch_dev reads.  Each listed key frame is computed as its own call would
 * compute it from the map as it stands.  That is exact for the key frame's own three members (mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames,
 * mvOrderedWeights): KFcounter depends on slots, observations and isBad() of points only, none of which UpdateConnections changes.  The reciprocal
 * AddConnection(this, w) on the other key frames (:522, :529) and the parent assignment (:549-554) are mutations in the reference's call order and stay the
 * caller's; the ordered row with its weights is exactly the list of those reciprocal calls.  Element for element under convention C.16:
 * ascending key-frame index stands for ascending KeyFrame*.
 * Counting (:461-479): every slot of the listed key frame (kf_mp_*) that is not NULL (negative) and not bad (mp_bad) adds 1 to each key frame of its
 * observation row (mp_obs_*), the listed key frame itself excepted (mnId == mnId: index equality); a point held in two slots counts twice; isBad() of the
 * observing key frames is not looked at; lines do not vote (:496 is commented out), so kf_ml_* and ml_bad are not read.  That a row of mp_obs_kf names a
 * key frame at most once (the keys of a std::map) is the caller's contract.
 * d_kf_list [n_list], or NULL for the key frames 0 .. n_list - 1; a key frame may be listed twice (it is computed twice).  th >= 1: the threshold of :508,
 * OLF_COVIS_TH in the reference.  Outputs per listed key frame j:
 *   d_n_counted [n_list]   KFcounter.size().  With 0 the reference returns at :501 and keeps the old members: here both rows of j are empty and
 *                          d_kf_max[j] = -1, d_w_max[j] = 0; keeping the old members stays the caller's.
 *   d_kf_max / d_w_max     pKFmax, nmax: the comparison at :514 is strict over ascending index, so the LOWEST index among the highest counts.
 *   d_conn_offsets [n_list + 1], d_conn_index / d_conn_weight [conn_capacity]     KFcounter as a CSR: every key frame with a count > 0 in ascending index --
 *                          mConnectedKeyFrameWeights (:545), GetConnectedKeyFrames().
 *   d_covis_offsets [n_list + 1], d_covis_index / d_covis_weight [covis_capacity] mvpOrderedConnectedKeyFrames / mvOrderedWeights: the key frames with count
 *                          >= th (:519), or, if there are none, the single pair (nmax, pKFmax) (:526-530); sorted as sort(vPairs) followed by push_front
 *                          leaves them (:532-539): descending weight, and among equal weights DESCENDING index -- the opposite tie rule to d_kf_max.
 *                          d_covis_index[d_covis_offsets[j]] is the parent candidate of :551; GetCovisiblesByWeight(w) is the prefix with weight >= w.
 * With d_kf_list == NULL and n_list == n_kf, d_covis_offsets / d_covis_index are kf_covis_offsets / kf_covis_index of an olf_map_graph as they are.
 * Both offset arrays are always complete; nothing is written at or past a capacity, and a total beyond one sets bit 16384 of the context's status word
 * (olf_ctx_synchronize / olf_ctx_poll_status).  Malformed indices are left out, never dereferenced: a slot index >= n_mp sets status bit 512, an
 * observation outside [0, n_kf) bit 4096; a listed key frame outside [0, n_kf) gets empty rows, d_n_counted 0, d_kf_max -1 and bit 4096.  Rows of a CSR are
 * clamped to [0, offsets[n]].
 * Errors: n_kf > OLF_LOCALMAP_MAX_KF (a key frame's vote table lives in LDS): OLF_ERR_CAPACITY before anything is launched; a NULL required pointer, a
 * negative size or th < 1: OLF_ERR_INVALID.  Of the graph only n_kf, n_mp, mp_obs_*, mp_bad and kf_mp_* are required; the other fields may be NULL.
 * n_list == 0 writes nothing.  Does not synchronise; runs on `stream` and uses the batch scratch slot: 4 bytes per (listed key frame, key frame of the
 * graph), the vote tables between its passes. */
#define OLF_COVIS_TH 15                        /* int th = 15, src/KeyFrame.cc:508 */
int olf_update_connections_batch_dev(olf_ctx* ctx, const olf_map_graph* g, int n_list, const int32_t* d_kf_list, int th, int32_t* d_n_counted, int32_t* d_kf_max,
                                     int32_t* d_w_max, int32_t* d_conn_offsets, int32_t* d_conn_index, int32_t* d_conn_weight, int conn_capacity,
                                     int32_t* d_covis_offsets, int32_t* d_covis_index, int32_t* d_covis_weight, int covis_capacity, void* stream);
/* host buffers, the graph's arrays included: checks mp_obs_* and kf_mp_* (offsets non-decreasing from 0: OLF_ERR_INVALID), uploads, runs the same kernels on
 * the context's stream, downloads.  OLF_ERR_CAPACITY when a capacity is too small: both offset arrays are complete then and each index / weight array holds
 * its first `capacity` entries; the same code, with the message of the bit, for a malformed index. */
int olf_update_connections(olf_ctx* ctx, const olf_map_graph* g, int n_list, const int32_t* kf_list, int th, int32_t* n_counted, int32_t* kf_max, int32_t* w_max,
                           int32_t* conn_offsets, int32_t* conn_index, int32_t* conn_weight, int conn_capacity, int32_t* covis_offsets, int32_t* covis_index,
                           int32_t* covis_weight, int covis_capacity);
/* void KeyFrame::UpdateBestCovisibles() (src/KeyFrame.cc:216-235) for n_rows rows of a CSR (d_conn_offsets [n_rows + 1], d_conn_index / d_conn_weight:
 * mConnectedKeyFrameWeights, e.g. the conn_* outputs above after the caller applied the reciprocal edges): every entry of a row is kept (no threshold), in
 * the order rule above (descending weight, among equal weights descending index), at the same offsets of d_covis_index / d_covis_weight.  Index values are
 * compared, not dereferenced, so nothing can be malformed; a row longer than OLF_LOCALMAP_MAX_KF sets status bit 16384 and is left unwritten.  Rows are
 * clamped to [0, offsets[n_rows]].  A NULL pointer or a negative n_rows: OLF_ERR_INVALID.  Does not synchronise; runs on `stream`, no scratch. */
int olf_best_covisibles_batch_dev(olf_ctx* ctx, int n_rows, const int32_t* d_conn_offsets, const int32_t* d_conn_index, const int32_t* d_conn_weight,
                                  int32_t* d_covis_index, int32_t* d_covis_weight, void* stream);

/* ---- LocalMapping::KeyFrameCulling, MapPointCulling and KeyFrame::TrackedMapPoints / TrackedMapLines (csrc/culling_batch.hip, culling_host.cpp) ---------
 * void LocalMapping::KeyFrameCulling() (src/LocalMapping.cc:632-696; called at :84) for a list of key frames -- GetVectorCovisibleKeyFrames() of the
 * current key frame, in its order -- against one snapshot of the map: an olf_map_graph and, beside it, an olf_cull_view (orbline_types.h).  It is not a
 * pure function of the snapshot: a culled key frame erases its observations (KeyFrame::SetBadFlag, src/KeyFrame.cc:647-649; MapPoint::EraseObservation,
 * src/MapPoint.cc:123-149), a point left with nObs <= 2 goes bad, and so a later key frame of the list can lose redundancy (its points have fewer
 * observers) or gain it (a point of its own that was not redundant went bad and nMPs fell).  As with the key-frame database, the data-parallel tables are
 * computed on the device (olf_keyframe_culling_tables_dev: every listed key frame against the map as it stands), the sequential rest is host code
 * (olf_keyframe_culling_replay) and a third entry runs both (olf_keyframe_culling).  The result is the reference's, decision for decision, in list order.
 * Integers only, apart from nRedundantObservations > 0.9 * nMPs (:693, one fp64 multiply, not contracted): exact equality, and no result depends on an
 * iteration order (the break at :680-681 only caps a count), so convention C.16 is not needed.
 *
 * olf_keyframe_culling_tables_dev.  Device pointers in g and v.  d_kf_list [n_list], or NULL for the key frames 0 .. n_list - 1; a key frame may be listed
 * twice.  monocular: mbMonocular.  Counting, :651-691:
 *   a slot COUNTS (nMPs++) when its point is not NULL (negative), not bad (mp_bad) and, unless monocular, not (depth > kf_th_depth || depth < 0) -- the
 *     comparisons as written, so a NaN depth counts;
 *   a counted slot is REDUNDANT when mp_nobs > 3 and at least 3 observations of its point qualify;
 *   an observation QUALIFIES when its key frame is not the listed one (index equality) and kf_slot_octave[kf_mp_offsets[kf_i] + slot_i] <= octave of this
 *     slot + 1: the observer's octave at the observation's slot (mp_obs_slot), the own octave at the slot that holds the point.  isBad() of an observer is
 *     not looked at; kf_bad, kf_mode and kf_slot_stereo are not read.
 * Outputs per listed key frame j: d_n_mps, d_n_redundant [n_list] (int32), d_redundant [n_list] (uint8) = (double)nRed > 0.9 * (double)nMPs.
 * Outputs per slot of the listed rows: d_row_offsets [n_list + 1], written here, the running sum of the listed rows' lengths (always complete); for slot i
 * of listed key frame j at d_row_offsets[j] + i: d_slot_count (int32), the UNCAPPED number of qualifying observations, also where mp_nobs <= 3 (the replay
 * needs it), and d_slot_flags (uint8), bit 0 counted, bit 1 redundant.  Every slot of a listed row is written; a slot that does not count gets 0 and 0.
 * The caller sizes the two slot arrays by the sum of the listed rows from its host copy of kf_mp_offsets and passes slot_capacity.  The list is a device
 * array, so a shortfall is found on the device: nothing is written at or past slot_capacity and bit 16384 of the context's status word is raised
 * (olf_ctx_synchronize / olf_ctx_poll_status); the per-key-frame outputs are complete all the same.  (olf_keyframe_culling, whose list is a host array,
 * sizes the arrays itself and cannot fall short.)
 * Malformed input is left out, never dereferenced: a slot index >= n_mp sets status bit 512; an observing key frame outside [0, n_kf), or an observation
 * slot outside that key frame's row, bit 4096 (the observation does not qualify); a listed key frame outside [0, n_kf) bit 4096, with zero counts and an
 * empty row.  An observation by the listed key frame itself is skipped before its slot is looked at.  Rows of a CSR are clamped to [0, offsets[n]].
 * There is no LDS table per key frame here, so OLF_LOCALMAP_MAX_KF does not apply: any n_kf.  Errors: a NULL required pointer (of g: mp_obs_offsets and
 * kf_mp_offsets; mp_obs_kf, mp_bad, mp_nobs and mp_obs_slot unless n_mp == 0; kf_mp_index, kf_slot_octave, kf_slot_depth and kf_th_depth unless n_kf == 0 --
 * an array without entries still needs an address) or a negative size: OLF_ERR_INVALID.
 * n_list == 0 writes nothing.  Does not synchronise; runs on `stream`; no scratch. */
int olf_keyframe_culling_tables_dev(olf_ctx* ctx, const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* d_kf_list, int monocular,
                                    int32_t* d_n_mps, int32_t* d_n_redundant, uint8_t* d_redundant, int32_t* d_row_offsets, int32_t* d_slot_count,
                                    uint8_t* d_slot_flags, int slot_capacity, void* stream);
/* The sequential rest, host only (no context): host copies of the graph, the view, the list (NULL: 0 .. n_list - 1) and the tables above.  Walks the list in
 * order; decision [n_list]:
 *   0  kept; also a key frame of mode 2 (skipped at :643) and one that was culled earlier in this list -- for these two n_mps / n_redundant are 0;
 *   1  culled: redundant and kf_mode 0, KeyFrame::SetBadFlag ran through;
 *   2  redundant but kf_mode 1: mbToBeErased is set, the map does not change (src/KeyFrame.cc:637-641).
 * n_mps / n_redundant [n_list]: nMPs and nRedundantObservations as the reference saw them at that moment.  After a decision 1 on key frame A the working
 * state changes as SetBadFlag changes the map: for every non-NULL slot of A whose point p is not bad and whose observation row names A (at slot s), the
 * observation is removed (once: a point held in two slots is erased at the first) and nobs[p] falls by 2 if kf_slot_stereo[A][s], else by 1 -- the
 * observation's slot, not the visiting one.  With nobs[p] <= 2 the point goes bad: every still undecided listed key frame that holds p in a counted slot
 * loses that slot from nMPs, and from nRed if it was redundant.  Otherwise every such slot loses one from its count if octave[A][s] <= its own octave + 1,
 * and is redundant again iff nobs > 3 && count >= 3.  The point -> (listed position, slot) index is built once from the listed rows.  That the slot an
 * observation names holds the observed point (AddObservation comes with AddMapPoint) and that an observation row names a key frame at most once are the
 * caller's contract: a point that goes bad leaves the counts through the slots that hold it.
 * Optional outputs (NULL: not wanted): mp_nobs_out, mp_bad_out [n_mp], the final counters and flags; went_bad [n_mp] / n_went_bad, the points that went
 * bad, in order.  Checks the two CSR pairs it reads and that row_offsets is the running sum of the listed rows' lengths (a listed key frame outside the
 * graph: an empty row, decision 0): OLF_ERR_INVALID otherwise, as for a NULL required pointer or a negative size.  Malformed indices are left out as above. */
int olf_keyframe_culling_replay(const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* kf_list, const int32_t* table_n_mps,
                                const int32_t* table_n_redundant, const int32_t* row_offsets, const int32_t* slot_count, const uint8_t* slot_flags,
                                int32_t* decision, int32_t* n_mps, int32_t* n_redundant, int32_t* mp_nobs_out, uint8_t* mp_bad_out, int32_t* went_bad,
                                int32_t* n_went_bad);
/* host buffers: checks mp_obs_* and kf_mp_* (offsets non-decreasing from 0: OLF_ERR_INVALID), sizes the slot arrays from the listed rows, uploads, runs the
 * tables on the context's stream, downloads, replays.  table_n_mps, table_n_redundant, table_redundant [n_list]: the tables' per-key-frame outputs, or
 * NULL.  OLF_ERR_CAPACITY with the message of the bit for a malformed index; the outputs are complete then. */
int olf_keyframe_culling(olf_ctx* ctx, const olf_map_graph* g, const olf_cull_view* v, int n_list, const int32_t* kf_list, int monocular, int32_t* decision,
                         int32_t* n_mps, int32_t* n_redundant, int32_t* table_n_mps, int32_t* table_n_redundant, uint8_t* table_redundant,
                         int32_t* mp_nobs_out, uint8_t* mp_bad_out, int32_t* went_bad, int32_t* n_went_bad);
/* int KeyFrame::TrackedMapPoints(minObs) and TrackedMapLines(minObs) (src/KeyFrame.cc:328-353, 407-432) for n_list key frames: the slots that are not NULL,
 * not bad and, with min_obs > 0 (bCheckObs), whose Observations() (d_mp_nobs [n_mp], d_ml_nobs [n_ml]) >= min_obs.  Tracking::NeedNewKeyFrame asks it of
 * every frame's reference key frame (src/Tracking.cc:1626-1627), which olf_update_local_map_batch_dev leaves on the device: its d_ref_kf is d_kf_list here
 * as it is.  A listed -1 is "no reference key frame": both counts 0 and no status bit.  Any other index outside [0, n_kf) gives 0 and bit 4096; a slot
 * index >= n_mp is left out with bit 512, a line index >= n_ml with bit 1024.  d_kf_list NULL: the key frames 0 .. n_list - 1.  A graph without lines
 * (kf_ml_offsets NULL) gives d_n_lines 0; d_ml_nobs may be NULL then, or when min_obs_lines <= 0; d_mp_nobs may be NULL when min_obs_points <= 0.
 * OLF_ERR_INVALID for a NULL required pointer or a negative size.  n_list == 0 writes nothing.  Does not synchronise; runs on `stream`; no scratch. */
int olf_tracked_map_points_batch_dev(olf_ctx* ctx, const olf_map_graph* g, const int32_t* d_mp_nobs, const int32_t* d_ml_nobs, int n_list,
                                     const int32_t* d_kf_list, int min_obs_points, int min_obs_lines, int32_t* d_n_points, int32_t* d_n_lines, void* stream);
/* host buffers: checks kf_mp_* and kf_ml_*, uploads, runs, downloads */
int olf_tracked_map_points(olf_ctx* ctx, const olf_map_graph* g, const int32_t* mp_nobs, const int32_t* ml_nobs, int n_list, const int32_t* kf_list,
                           int min_obs_points, int min_obs_lines, int32_t* n_points, int32_t* n_lines);
/* void LocalMapping::MapPointCulling() (src/LocalMapping.cc:170-205; called at :64) as a predicate over the n points of mlpRecentAddedMapPoints, given as
 * arrays: d_bad (uint8, isBad()), d_found / d_visible (int32, mnFound / mnVisible), d_nobs (int32, Observations()), d_first_kf_id (int64, mnFirstKFid);
 * current_kf_id = mpCurrentKeyFrame->mnId.  d_action [n] (uint8), the branches of :186-203 in their order:
 *   1  erase from the list (bad);  2  SetBadFlag and erase: GetFoundRatio() = (float)found / (float)visible < 0.25f (visible == 0 gives NaN or inf and
 *   falls through, as in the reference);  3  SetBadFlag and erase: (int)current - (int)first >= 2 && nobs <= (monocular ? 2 : 3);  4  erase: that
 *   difference >= 3;  0  keep.
 * A NULL pointer with n > 0 or a negative n: OLF_ERR_INVALID.  n == 0 writes nothing.  Does not synchronise; runs on `stream`; no scratch. */
int olf_map_point_culling_dev(olf_ctx* ctx, int n, const uint8_t* d_bad, const int32_t* d_found, const int32_t* d_visible, const int32_t* d_nobs,
                              const int64_t* d_first_kf_id, int64_t current_kf_id, int monocular, uint8_t* d_action, void* stream);
/* host buffers: uploads, runs, downloads */
int olf_map_point_culling(olf_ctx* ctx, int n, const uint8_t* bad, const int32_t* found, const int32_t* visible, const int32_t* nobs,
                          const int64_t* first_kf_id, int64_t current_kf_id, int monocular, uint8_t* action);

/* ---- the entries that produce map arrays: ComputeF12 and UpdateNormalAndDepth (csrc/newpoints_batch.hip, newpoints_host.cpp, newpoints_terms.hpp) ----------
 * cv::Mat LocalMapping::ComputeF12(KeyFrame *&pKF1, KeyFrame *&pKF2) (src/LocalMapping.cc:536-553; called at :264) for n_pairs pairs of the n_frames
 * frames of a batch: d_F12 of olf_search_for_triangulation_batch_dev for the same d_pairs, without a host step.  `in`: only Tcw and fx, fy, cx, cy are
 * read (both key frames share mK).  R12 = R1w * R2w.t() (a transposed operand: double accumulation, one rounding), t12 = -R1w * R2w.t() * t2w + t1w (the
 * negated R12, then a plain product with t1w as its C term), K1.t().inv() * t12x * R12 * K2.inv() left to right as three plain products (C.12);
 * cv::invert of the two 3 x 3 matrices is the closed-form adjugate with determinant and cofactors in double, one rounding per element (C.18).
 * d_pairs [n_pairs][2] = (kf1, kf2); d_F12 [n_pairs][9] row-major, used as x1^T F12 x2.  A pair whose index lies outside [0, n_frames), or with
 * kf1 == kf2, is left untouched and sets bit 2048 of the context's status word.  n_pairs == 0 writes nothing; a NULL required pointer or a negative
 * count: OLF_ERR_INVALID, before any launch.  Does not synchronise; runs on `stream`; no scratch. */
int olf_compute_f12_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, float* d_F12, void* stream);
/* the host form: one pair from its two 4 x 4 poses (row-major), no context and no device; the same text (csrc/newpoints_terms.hpp) */
int olf_compute_f12(const float* Tcw1, const float* Tcw2, float fx, float fy, float cx, float cy, float* F12);
/* void LocalMapping::CreateNewMapPoints() after the search (src/LocalMapping.cc:245-253 and :286-431: the baseline test, the parallax test, linear
 * triangulation or KeyFrame::UnprojectStereo, the depth, reprojection and scale gates) for n_pairs pairs (kf1 = mpCurrentKeyFrame, kf2 = a neighbour) of
 * the n_frames frames of a batch and the match rows exactly as olf_search_for_triangulation_batch_dev wrote them: d_matches12 [n_pairs][capacity], row p
 * holding per idx1 the idx2 or -1.  `in`: kps (mvKeysUn), counts, img_stride, uright, Tcw and fx, fy, cx, cy, mbf are read; d_depth [n_frames][capacity]
 * is mvDepth (as olf_unproject_stereo_dev takes it); mb = mbf / fx as the key frames hold it; mvScaleFactors / mvLevelSigma2 are the context's, and
 * ratioFactor = 1.5f * mvScaleFactors[1] (mfScaleFactor; 1 in a context of one level).  monocular: mbMonocular -- 0 applies the `baseline < pKF2->mb`
 * skip of :249-253, 1 skips nothing here (ComputeSceneMedianDepth stays the caller's).
 * Outputs, one row per pair, indexed by idx1: d_x3D [n_pairs][capacity][3], the new point where d_code is 1 to 3 and zeros elsewhere; d_code
 * [n_pairs][capacity] (uint8):
 *    0  no match (also from N1 on)           1  created by triangulation
 *    2  created by UnprojectStereo of kf1    3  created by UnprojectStereo of kf2
 *   16  low parallax without stereo (:349)  17  w == 0 (:334)      18  z1 <= 0 (:356)             19  z2 <= 0 (:360)
 *   20  reprojection in kf1 (:375, :386)    21  reprojection in kf2 (:401, :412)    22  dist1 == 0 || dist2 == 0 (:423)    23  scale ratio (:431)
 * d_nnew [n_pairs]: the number of codes 1 to 3 of the row, `nnew` of the pair.  A pair skipped by the baseline test has nnew = 0 and an all-0 row.  What
 * follows a created point in the reference (new MapPoint, AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth) is the
 * caller's, from the codes; olf_update_normal_and_depth_dev is the last of them.  One call over all pairs is the snapshot answer: see INTEGRATION.md for
 * the reference's neighbour-by-neighbour staleness.
 * Arithmetic (csrc/newpoints_terms.hpp, one text for this entry and its host form; C.12 products, C.4 no contraction): cosParallaxRays is a double quotient
 * of Mat::dot and two cv::norm rounded to float; cos(2 * atan2(mb / 2, depth)) is the float overloads, glibc's atan2f and cosf as csrc/device_math.hpp
 * restates them; the rows of A are a float product and a float difference per element; cv::SVD::compute is the float one-sided Jacobi iteration of an
 * OpenCV built without LAPACK (C.19: a build with LAPACK calls sgesdd and differs in the last bits; the tests compare triangulated points by tolerance);
 * x3D / w multiplies by (float)(1.0 / (double)w) (C.17); z = Rcw.row(2).dot(x3Dt) + tcw(2) is a double sum rounded once; invz = (float)(1.0 / z); the
 * error sums are float, compared with the double products 5.991 * sigma2 and 7.8 * sigma2; the right-image term of BOTH key frames uses mbf of the
 * current one (:406, as written); UnprojectStereo is the routine of olf_unproject_stereo_dev on Twc = [Rcw.t() | Ow], Ow = -Rwc * tcw as KeyFrame::SetPose
 * forms it (src/KeyFrame.cc:154-155: a plain product on the materialised transpose).  A feature with mvuRight >= 0 and mvDepth <= 0, for which the
 * reference's UnprojectStereo returns an empty matrix, is computed with that depth.
 * Malformed input: a pair with an index outside [0, n_frames) or kf1 == kf2 gives nnew = -1, leaves its rows untouched and sets bit 2048 of the context's
 * status word; an idx2 outside [0, N2) is no match; a match either of whose key points holds an octave outside the context's levels is left out (code 0)
 * with bit 256.  n_pairs == 0 writes nothing; a NULL required pointer or a negative count: OLF_ERR_INVALID, before any launch.  Nothing is read or
 * written out of bounds.  Results do not depend on scheduling or on a pair's position in the list.  Does not synchronise; runs on `stream`; no scratch. */
int olf_create_new_map_points_batch_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const float* d_depth, float mb, int n_pairs, const int32_t* d_pairs,
                                        const int32_t* d_matches12, int monocular, float* d_x3D, uint8_t* d_code, int32_t* d_nnew, void* stream);
/* the host form: host pointers in `in` and everywhere else, no context and no device; capacity: the row length of the per-frame planes; scale_factors
 * [n_levels] = mvScaleFactors; *status receives the bits 256 / 2048 */
int olf_create_new_map_points(const olf_track_batch* in, int capacity, int n_frames, const float* depth, float mb, const float* scale_factors, int n_levels,
                              int n_pairs, const int32_t* pairs, const int32_t* matches12, int monocular, float* x3D, uint8_t* code, int32_t* nnew,
                              int32_t* status);
/* void MapPoint::UpdateNormalAndDepth() (src/MapPoint.cc:342-383; called for new points at src/LocalMapping.cc:444, for fused points at :527, after every bundle
 * adjustment, src/Optimizer.cc:227, :1743, :2009, in loop correction, src/LoopClosing.cc:506, and at map load, src/Map.cc:665) for n_points map points of one snapshot: d_points [n_points], or NULL for the points 0 .. n_points - 1
 * (n_points = n_mp: every point).  Reads mp_obs_offsets, mp_obs_kf, mp_bad and kf_mp_offsets of g, mp_obs_slot and kf_slot_octave of v (device pointers),
 * d_mp_world [n_mp][3] (mWorldPos), d_mp_ref_kf [n_mp] (mpRefKF as a key-frame index) and d_kf_Ow [n_kf][3] (GetCameraCenter()); mvScaleFactors and
 * mnScaleLevels are the context's.  Writes, in place and only for the listed points: d_normal [n_mp][3] (mNormalVector), d_maxd, d_mind [n_mp]
 * (mfMaxDistance, mfMinDistance: unscaled, as olf_local_map takes them).  A bad point (:350) or a point with an empty observation row (:357) is left
 * untouched.
 * The normal is summed over the observation row IN ROW ORDER, sequentially in float (:362-369).  The reference iterates a std::map<KeyFrame*, size_t>,
 * i.e. in address order: a caller who wants convention C.15 / C.16 (ascending key-frame index stands for ascending address) passes every row ascending.
 * normali / cv::norm(normali) multiplies by (float)(1.0 / norm) with the norm kept in double, normal / n by (float)(1.0 / (double)n) (C.17).
 * mfMaxDistance = (float)cv::norm(Pos - Ow_ref) * mvScaleFactors[level], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1], in float.  The level
 * is the octave at slot observations[pRefKF] of the reference key frame (:373): the slot of the row's entry that names d_mp_ref_kf, or, when the row does
 * not name it, slot 0 -- std::map::operator[] inserts a zero there and the reference reads mvKeysUn[0].octave.
 * Malformed input is left out, never dereferenced: an observation whose key frame lies outside [0, n_kf) or whose slot lies outside that key frame's row
 * sets bit 4096 of the context's status word and enters neither the sum, nor n, nor the search for the reference's slot (a point left without
 * observations counts as an empty row); a reference key frame outside [0, n_kf), or a level slot outside the reference's row, sets bit 4096 and leaves
 * the point untouched; an octave outside the context's levels does so with bit 256; a point index outside [0, n_mp) with bit 512.  A point listed twice
 * is computed twice with the same result.  Errors: a NULL required pointer (mp_obs_offsets, kf_mp_offsets; the per-point arrays unless n_mp == 0; the
 * per-key-frame arrays unless n_kf == 0) or a negative size: OLF_ERR_INVALID.  n_points == 0 writes nothing.  Does not synchronise; runs on `stream`; no
 * scratch. */
int olf_update_normal_and_depth_dev(olf_ctx* ctx, const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* d_points, const float* d_mp_world,
                                    const int32_t* d_mp_ref_kf, const float* d_kf_Ow, float* d_normal, float* d_maxd, float* d_mind, void* stream);
/* the host form: host pointers, no context and no device; scale_factors [n_levels] = mvScaleFactors (olf_orb_scale_tables), 1 <= n_levels <=
 * OLF_MAX_LEVELS; *status receives the bits 256 / 512 / 4096.  Checks the two offsets arrays (non-decreasing from 0: OLF_ERR_INVALID otherwise). */
int olf_update_normal_and_depth(const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* points, const float* mp_world,
                                const int32_t* mp_ref_kf, const float* kf_Ow, const float* scale_factors, int n_levels, float* normal, float* maxd, float* mind,
                                int32_t* status);

/* The three entries above from host pointers ON THE DEVICE (csrc/newpoints_api.cpp): the arrays are staged, the same kernels run on the context's stream,
 * the outputs come back; synchronises.  The outputs are uploaded first, so what the device form leaves untouched (a refused pair's rows, a bad point) comes
 * back as it went in.  The per-frame planes of `in` and depth are [n_frames][olf_orb_capacity(ctx)], as for the device forms; Tcw [n_frames][16].  The
 * update entry checks the two offsets arrays (non-decreasing from 0: OLF_ERR_INVALID).  A set status bit makes the call return OLF_ERR_CAPACITY with the
 * bit's text, the outputs complete. */
int olf_compute_f12_pairs(olf_ctx* ctx, const float* Tcw, int n_frames, float fx, float fy, float cx, float cy, int n_pairs, const int32_t* pairs, float* F12);
int olf_create_new_map_points_pairs(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const float* depth, float mb, int n_pairs, const int32_t* pairs,
                                    const int32_t* matches12, int monocular, float* x3D, uint8_t* code, int32_t* nnew);
int olf_update_normal_and_depth_points(olf_ctx* ctx, const olf_map_graph* g, const olf_cull_view* v, int n_points, const int32_t* points, const float* mp_world,
                                       const int32_t* mp_ref_kf, const float* kf_Ow, float* normal, float* maxd, float* mind);

/* ---- Tracking::NeedNewKeyFrame and the three producers of stereo landmarks for a batch on the device (csrc/keyframe_batch.hip) --------------------------
 * Which stereo features of a frame get a new map point or map line, in which order, and what the new landmark holds -- the loops of
 *   OLF_LANDMARKS_INIT       Tracking::StereoInitialization (src/Tracking.cc:639-677): every point with z > 0 and every line whose two disparities are
 *                            > 0, in index order; no sort, held entries are not consulted
 *   OLF_LANDMARKS_KEYFRAME   Tracking::CreateNewKeyFrame (:1744-1865)
 *   OLF_LANDMARKS_LASTFRAME  Tracking::UpdateLastFrame (:1092-1204), with its early return: a frame without a stereo point visits no line (:1105-1106)
 * for n_frames device-resident frames; frame j = image j * img_stride of kps / counts / kls / lcounts (as olf_track_batch and olf_line_batch), every other
 * plane is per frame.  Each frame is answered on its own, from the arrays as they stand (a snapshot answer).
 * The two sorted modes: vDepthIdx holds (z, i) for the points with z > 0 (:1749-1756), for the lines (max(sz, ez), i) with sz = mbf / disparity in float
 * unless sz < 0 || ez < 0 (:1806-1813: a disparity of -1 or -0.0f is skipped, +0.0f gives +inf and is kept); std::sort by pair's operator<, a total
 * order, so the result is the order of the 64-bit keys (bits of z << 32 | i); the walk visits entries until the first one with z > thDepth once more
 * than 100 (lines: 50) have been visited (:1796, :1862: the test comes after the visit and nPoints counts both branches), i.e. the first
 * min(n, max(nClose, 100) + 1) entries, nClose = the number of entries with !(z > thDepth).  A visited feature gets a new landmark when it holds none or
 * one with Observations() < 1 (:1769-1776, :1119-1125).
 * The new landmarks.  Points: mp_world = Frame::UnprojectStereo, the routine of olf_unproject_stereo_dev on Twc (rows of mRwc | mOw).  mp_normal,
 * mp_maxd, mp_mind with Ow = column 3 of Twc: in LASTFRAME mode the constructor MapPoint(Pos, pMap, pFrame, idxF) (src/MapPoint.cc:58-83): normal =
 * (Pos - Ow) * (float)(1.0 / cv::norm) (C.17); in the other two modes MapPoint::UpdateNormalAndDepth of a point with the one observation (zeros + that
 * vector, times (float)(1.0 / 1): a -0 component becomes +0; a caller who wants the key frame's own camera centre passes Twc = [Rcw.t() | Ow] of
 * KeyFrame::SetPose).  mfMaxDistance = (float)cv::norm(Pos - Ow) * mvScaleFactors[octave], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1].
 * Lines: Frame::backProjection (src/Frame.cc:1089-1098) of both endpoints in double (C.29): bd = (double)mb / (double)disp with mb the float mbf / fx;
 * P = (bd * (u - cx), bd * (v - cy), bd * fx) with the floats widened; Rwc * P + Ow summed over k ascending, without contraction.  ml_world_d holds the
 * doubles, ml_world their Converter::toCvMat (one rounding to float), the layout of olf_local_line_map.world.
 * Outputs per frame j (all planes are written for every feature slot of the frame, whatever the count):
 *   n_visited [2], n_created [2]       points, lines: the final nPoints / nLines (INIT: the number created) and the number of new landmarks
 *   visit_order, visit_order_l         feature indices in visit order, -1 past the end
 *   created_order, created_order_l     the created subset in visit order (the order of mnId and of mlpTemporalPoints / mlpTemporalLines), -1 past the end
 *   created, created_l                 1 where a landmark was created, by feature index: mp_valid of olf_track_batch for the temporal points
 *   frame_mp_out, frame_ml_out         mvpMapPoints / mvpMapLines after the loop: new_base[j] + k for the k-th created of the frame (new_base_* NULL:
 *                                      n_mp / n_ml), the input entry elsewhere (-1 where frame_mp / frame_ml is NULL)
 *   mp_world, mp_normal [.][3], mp_maxd, mp_mind; ml_world_d (or NULL), ml_world [.][6]      by feature index, zeros where nothing was created
 *   status                             the frame's own word: 1 a line depth that is NaN (std::sort is undefined there: the frame's line outputs are
 *                                      empty); 2 a held index >= n_mp / n_ml (treated as NULL); 4 a created point whose octave is outside the
 *                                      context's levels (maxd = mind = 0)
 * A count beyond the capacity is read as the capacity.  frame_mp / frame_ml NULL: nothing is held; mp_nobs / ml_nobs (Observations()) are read only for
 * held entries.  n_frames == 0 writes nothing.  Contexts above OLF_GRID_MAX_KEYS key points or key lines: OLF_ERR_CAPACITY; a NULL required pointer,
 * n_frames < 0, img_stride < 1, n_mp or n_ml < 0 or an unknown mode: OLF_ERR_INVALID.  Does not synchronise; runs on `stream`; no scratch; the context's
 * status word is not touched.  Results do not depend on scheduling. */
enum { OLF_LANDMARKS_INIT = 0, OLF_LANDMARKS_KEYFRAME = 1, OLF_LANDMARKS_LASTFRAME = 2 };
typedef struct olf_landmarks_batch {
    const olf_keypoint* kps; const int32_t* counts;      /* mvKeysUn, N                                                   */
    const olf_keyline*  kls; const int32_t* lcounts;     /* mvKeysUn_Line, N_l                                            */
    int32_t img_stride;
    const float*   depth;          /* [n_frames][capacity] mvDepth                                                       */
    const float*   ldisp;          /* [n_frames][line capacity][2] mvDisparity_l                                         */
    const float*   Twc;            /* [n_frames][16] rows of mRwc | mOw (olf_unproject_stereo_dev)                        */
    const int32_t* frame_mp;       /* [n_frames][capacity] mvpMapPoints as map indices, negative = NULL; or NULL         */
    const int32_t* frame_ml;       /* [n_frames][line capacity] mvpMapLines; or NULL                                      */
    const int32_t* mp_nobs; int32_t n_mp;                /* Observations() of the n_mp map points                         */
    const int32_t* ml_nobs; int32_t n_ml;
    const int32_t* new_base_mp;    /* [n_frames] index of the frame's first new point; NULL: n_mp for every frame         */
    const int32_t* new_base_ml;    /* [n_frames]; NULL: n_ml                                                               */
    float fx, fy, cx, cy, mbf, thDepth;
} olf_landmarks_batch;
typedef struct olf_landmarks_outputs {
    int32_t* n_visited; int32_t* n_created;              /* [n_frames][2]                                                  */
    int32_t* visit_order; int32_t* visit_order_l;        /* [n_frames][capacity], [n_frames][line capacity]                */
    int32_t* created_order; int32_t* created_order_l;
    uint8_t* created; uint8_t* created_l;
    int32_t* frame_mp_out; int32_t* frame_ml_out;
    float* mp_world; float* mp_normal; float* mp_maxd; float* mp_mind;
    double* ml_world_d; float* ml_world;                 /* ml_world_d may be NULL                                         */
    int32_t* status;                                     /* [n_frames]                                                     */
} olf_landmarks_outputs;
int olf_stereo_landmarks_batch_dev(olf_ctx* ctx, const olf_landmarks_batch* in, int n_frames, int mode, const olf_landmarks_outputs* out, void* stream);
/* the host form: host pointers, no context and no device; capacity / line_capacity: the row lengths of the per-frame planes (at most OLF_GRID_MAX_KEYS);
 * scale_factors [n_levels] = mvScaleFactors, 1 <= n_levels <= OLF_MAX_LEVELS.  The same text (csrc/keyframe_terms.hpp). */
int olf_stereo_landmarks(const olf_landmarks_batch* in, int capacity, int line_capacity, int n_frames, int mode, const float* scale_factors, int n_levels,
                         const olf_landmarks_outputs* out);
/* bool Tracking::NeedNewKeyFrame() (src/Tracking.cc:1606-1725) for n_frames frames.  The four counts of :1632-1667 come from the frame's planes: a point
 * with 0 < mvDepth < thDepth is tracked when it holds a map point and is no outlier, else untracked; a line with minz > 0 && maxz < thDepth (minz, maxz =
 * the ordered mbf / disparity of its endpoints, in float) likewise.  The line loop reads mLastFrame.mvDisparity_l[i] for i < mCurrentFrame.N_l
 * (:1651-1652, as written): row j reads the disparities of frame ldisp_frame[j] (NULL: j itself; the reference as written: j - 1).  An i at or beyond
 * that frame's line count -- where the reference reads out of bounds -- is not counted and sets bit 1 of the row's status; so is every line when
 * ldisp_frame[j] is outside [0, n_frames).  A monocular row counts nothing (:1637).
 * The decision (:1609-1724) is one function of csrc/keyframe_terms.hpp in the reference's types: frame ids are unsigned, mnLastKeyFrameId + mMaxFrames
 * wraps at 32 bits; mnMatchesInliers < nRefMatches * 0.25 compares in double, mnMatchesInliers < nRefMatches * thRefRatio in float.  rows [n_frames][11]
 * (int32): mnId, mnLastKeyFrameId, mnLastRelocFrameId, mMinFrames, mMaxFrames, nKFs (KeyFramesInMap()), bLocalMappingIdle (AcceptKeyFrames()),
 * KeyframesInQueue(), mbOnlyTracking, stopped (isStopped() || stopRequested()), monocular.  n_ref_matches, n_ref_matches_l [n_frames]: the outputs of
 * olf_tracked_map_points_batch_dev as they are (no reference key frame: 0); n_inliers [n_frames][2]: that of olf_pose_outputs as it is
 * (mnMatchesInliers, mnMatchesInliers_l).
 * Outputs per frame: need (the return value), interrupt_ba (1: InterruptBA() was called, :1711), counts [4] = nTrackedClose, nNonTrackedClose,
 * nTrackedClose_l, nNonTrackedClose_l; conditions = c1a | c1b << 1 | c1c << 2 | c1c_l << 3 | c2 << 4 | c2_l << 5 (0 when an early return came first);
 * status.  outlier / outlier_l NULL: none; frame_mp / frame_ml NULL: nothing is held (any value >= 0 counts as held).  A count beyond the capacity is
 * read as the capacity.  n_frames == 0 writes nothing; a NULL required pointer, n_frames < 0 or img_stride < 1: OLF_ERR_INVALID; contexts above
 * OLF_GRID_MAX_KEYS: OLF_ERR_CAPACITY.  Does not synchronise; runs on `stream`; no scratch. */
#define OLF_KEYFRAME_ROW 11
typedef struct olf_keyframe_test_batch {
    const int32_t* counts; const int32_t* lcounts; int32_t img_stride;      /* N, N_l                                    */
    const float*   depth;  const int32_t* frame_mp; const uint8_t* outlier;       /* mvDepth, mvpMapPoints, mvbOutlier          */
    const float*   ldisp;  const int32_t* frame_ml; const uint8_t* outlier_l;     /* mvDisparity_l, mvpMapLines, mvbOutlier_Line */
    const int32_t* ldisp_frame;
    const int32_t* rows; const int32_t* n_ref_matches; const int32_t* n_ref_matches_l; const int32_t* n_inliers;
    float mbf, thDepth;
} olf_keyframe_test_batch;
typedef struct olf_keyframe_test_outputs {
    uint8_t* need; uint8_t* interrupt_ba;                /* [n_frames]                                                      */
    int32_t* counts;                                     /* [n_frames][4]                                                   */
    int32_t* conditions; int32_t* status;                /* [n_frames]                                                      */
} olf_keyframe_test_outputs;
int olf_need_new_keyframe_batch_dev(olf_ctx* ctx, const olf_keyframe_test_batch* in, int n_frames, const olf_keyframe_test_outputs* out, void* stream);
/* the host form: host pointers, no context and no device; capacity / line_capacity: the row lengths of the per-frame planes */
int olf_need_new_keyframe(const olf_keyframe_test_batch* in, int capacity, int line_capacity, int n_frames, const olf_keyframe_test_outputs* out);
/* The two device entries from host pointers ON THE DEVICE (csrc/keyframe_api.cpp): the arrays are staged, the same kernels run on the context's stream,
 * the outputs come back; synchronises.  The planes are [n_frames * img_stride] or [n_frames] rows of the context's capacities. */
int olf_stereo_landmarks_frames(olf_ctx* ctx, const olf_landmarks_batch* in, int n_frames, int mode, const olf_landmarks_outputs* out);
int olf_need_new_keyframe_frames(olf_ctx* ctx, const olf_keyframe_test_batch* in, int n_frames, const olf_keyframe_test_outputs* out);

/* ---- Sim3Solver's RANSAC for a list of key-frame pairs on the device (csrc/sim3solver_batch.hip) ------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) as LoopClosing::ComputeSim3 drives it per candidate (src/LoopClosing.cc:280-307): the constructor's
 * correspondences, SetRansacParameters(probability, min_inliers, max_iterations) and one iterate(n_iterations, ...) per call, for n_pairs pairs of the
 * n_frames key frames of a batch.  It stands between olf_search_by_bow_pairs_dev (form OLF_BOW_KF_KF), whose rows it reads, and
 * olf_search_by_sim3_pairs_dev, which takes best_s / best_R / best_t as its d_s12 / d_R12 / d_t12 without a copy; olf_sim3_filter_matches_dev does
 * :319-324 between them.  Optimizer::OptimizeSim3 (:332) is olf_optimize_sim3_pairs_dev below.  Results equal olf_sim3_solver pair by pair, bit for bit, and do not depend
 * on scheduling, on how the kernel chunks a window or on a pair's position in the list.
 * `in`: kps (octave), counts, img_stride, Tcw, mp_world, mp_valid (NULL: every feature holds a point) and fx, fy, cx, cy are read (frame j = image
 * j * img_stride; a count beyond the capacity is read as the capacity); mvLevelSigma2 is the context's.  d_mp_bad [n_frames][capacity] (or NULL: none is
 * bad): isBad() of the point a feature holds.  d_pairs [n_pairs][2] = (kf1, kf2).  d_matches12 [n_pairs][capacity], read only: exactly the row
 * olf_search_by_bow_pairs_dev writes or olf_search_by_sim3_pairs_dev has extended; value v at i1 < N1 is a correspondence iff 0 <= v < N2 (-1, -2 and
 * >= N2 are all "none"), both features hold a point and neither point is bad; indexKF1 = i1, indexKF2 = v.  Correspondences are kept in ascending i1.
 * The gates are integers: (size_t)(9.210 * sigmaSquare) (level 0: 9, level 1 at 1.2: 13), compared as float.  A correspondence either of whose octaves
 * lies outside the context's levels is left out and sets bit 256 of the context's status word.
 * olf_sim3_ransac: fix_scale (bFixScale), probability in (0, 1), min_inliers >= 3, max_iterations >= 1 (the reference: 0.99, 20, 300), n_iterations >= 0:
 * the window of this call (the reference: 5; max_iterations gives find()).  The iteration cap is a function of the number of correspondences alone; the
 * call computes it for every N in [0, capacity] on the host with the host's libm (csrc/sim3solver_terms.hpp: s3_iteration_cap) and the kernel looks it up.
 * d_draws [n_pairs][max_iterations][3] (uint32): the raw rand() values below 2^31 of every iteration, indexed by ABSOLUTE iteration, so a resumed call
 * reads on where the last one stopped (convention C.20; bit 31 of a value is ignored); draw k picks position (int)(((double)r / 2147483648.0) * (N - k)) of what is still available.
 * olf_sim3_solver_io, device pointers, one element or row per pair.  In and out -- the solver's carried state, all zero for a new solver:
 * iterations_done (mnIterations), best_inliers (mnBestInliers), best_s, best_R [9], best_t [3], best_T12 [16] (row-major).  An iteration with
 * n >= best_inliers replaces them; the first that also has n > min_inliers is accepted and ends the call (:183-200).  Out: accepted (the returned Scm is
 * not empty), no_more (bNoMore), n_inliers (0 unless accepted), inliers [n_pairs][capacity] (uint8, indexed by i1; positions below N1 are written, all 0
 * unless accepted; positions from N1 on are left as they are), n_correspondences (N), and counts [n_pairs][max_iterations] (may be NULL): the inlier
 * count of every iteration this call evaluated at its absolute index, the others untouched.  N < min_inliers: no_more = 1 and the state is untouched.
 * Arithmetic (csrc/sim3solver_terms.hpp and, for the sample of C.20, ransac_terms.hpp: one text for this entry and its host form; C.4, C.12, C.17,
 * C.20 to C.22 of DESIGN.md).
 * A pair whose index lies outside [0, n_frames), or with kf1 == kf2, gets n_inliers = -1, nothing else of it is written, and bit 2048 is set.  Errors,
 * before any launch: a NULL required pointer, a negative count, min_inliers < 3, max_iterations < 1, n_iterations < 0 or probability outside (0, 1):
 * OLF_ERR_INVALID.  n_pairs == 0 writes nothing.  Does not synchronise; runs on `stream`.  Nothing is read or written out of bounds.
 * Scratch: 4 bytes per feature of the capacity and, where 52 bytes per feature of the capacity exceed the LDS a workgroup takes, that much per resident
 * workgroup (at most 1024). */
typedef struct olf_sim3_ransac {
    int32_t fix_scale;
    double  probability;
    int32_t min_inliers, max_iterations, n_iterations;
} olf_sim3_ransac;
typedef struct olf_sim3_solver_io {
    int32_t* iterations_done;    /* [n_pairs]      in / out */
    int32_t* best_inliers;       /* [n_pairs]      in / out */
    float*   best_s;             /* [n_pairs]      in / out: d_s12 of olf_search_by_sim3_pairs_dev */
    float*   best_R;             /* [n_pairs][9]   in / out: d_R12 */
    float*   best_t;             /* [n_pairs][3]   in / out: d_t12 */
    float*   best_T12;           /* [n_pairs][16]  in / out */
    int32_t* accepted;           /* [n_pairs] */
    int32_t* no_more;            /* [n_pairs] */
    int32_t* n_inliers;          /* [n_pairs] */
    uint8_t* inliers;            /* [n_pairs][capacity] */
    int32_t* n_correspondences;  /* [n_pairs] */
    int32_t* counts;             /* [n_pairs][max_iterations], or NULL */
} olf_sim3_solver_io;
int olf_sim3_solver_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                              const int32_t* d_matches12, const olf_sim3_ransac* ransac, const uint32_t* d_draws, const olf_sim3_solver_io* io, void* stream);
/* LoopClosing.cc:319-324 for every pair: d_out[p][i] = d_matches12[p][i] where d_inliers[p][i] is set, -1 elsewhere, for i in [0, capacity).  d_out may be
 * d_matches12 itself.  d_n_inliers (or NULL) [n_pairs]: a pair with a negative value (a refused pair) keeps its row of d_out.  Does not synchronise. */
int olf_sim3_filter_matches_dev(olf_ctx* ctx, int n_pairs, const int32_t* d_matches12, const uint8_t* d_inliers, const int32_t* d_n_inliers, int32_t* d_out,
                                void* stream);
/* the host form: ONE pair (kf1, kf2), host pointers in `in` and everywhere else, no context and no device, the literal loop of Sim3Solver::iterate.
 * capacity: the row length of the per-frame planes; scale_factors [n_levels] = mvScaleFactors; matches12 [capacity], draws [max_iterations][3]; every
 * pointer of io names this pair's element or row; *status receives the bits 256 / 2048. */
int olf_sim3_solver(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* scale_factors, int n_levels, int kf1, int kf2,
                    const int32_t* matches12, const olf_sim3_ransac* ransac, const uint32_t* draws, const olf_sim3_solver_io* io, int32_t* status);
/* olf_sim3_solver_pairs_dev from host pointers ON THE DEVICE (csrc/sim3solver_api.cpp): the arrays are staged (the in / out state and the outputs are
 * uploaded first), the same kernel runs on the context's stream, state and outputs come back; synchronises.  A set status bit makes the call return
 * OLF_ERR_CAPACITY with the bit's text, the outputs complete. */
int olf_sim3_solver_pairs(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* mp_bad, int n_pairs, const int32_t* pairs,
                          const int32_t* matches12, const olf_sim3_ransac* ransac, const uint32_t* draws, const olf_sim3_solver_io* io);
/* tests: the LDS a workgroup of the solver may take for its correspondences (bytes; above it they live in context scratch; <= 0 restores the default),
 * and the integer gate of a level's scale factor */
int olf_debug_sim3_solver_lds_limit(int bytes);
int olf_debug_sim3_solver_gate(float scale_factor, uint64_t* gate);
/* tests: the iteration cap the solver's table holds for N correspondences (csrc/sim3solver_terms.hpp: s3_iteration_cap) */
int olf_debug_sim3_solver_cap(int N, double probability, int min_inliers, int max_iterations, int32_t* cap);

/* ---- Optimizer::OptimizeSim3 for a list of key-frame pairs on the device (csrc/optsim3_batch.hip, optsim3_host.cpp, optsim3_terms.hpp) ------------------
 * int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches1, g2o::Sim3 &g2oS12, const float th2, const bool bFixScale)
 * (src/Optimizer.cc:2013-2208), called per loop candidate by LoopClosing::ComputeSim3 (src/LoopClosing.cc:332): the g2o graph of one free
 * VertexSim3Expmap and, per correspondence in ascending i, one EdgeSim3ProjectXYZ and one EdgeInverseSim3ProjectXYZ against fixed camera-frame points,
 * Huber kernels of the float delta sqrt(th2), optimize(5), the chi2 check against th2 that removes a failing correspondence's two edges and nulls its
 * match, the `< 10` gate, optimize(10 or 5) from the current estimate, the final check.  The edges have no analytic Jacobian in the reference, so every
 * linearisation differentiates numerically (14 perturbed estimates); that and every other term is csrc/optsim3_terms.hpp, one text for the host form
 * and the kernel (C.4, C.27, C.28 of DESIGN.md).  The stale-error quirk of olf_pose_optimization_batch_dev holds here too: a check reads the _error the
 * last computeActiveErrors() left, the rejected estimate's after a rejected last trial.
 * The entry takes exactly what olf_search_by_sim3_pairs_dev took and wrote: `in`, d_mp_bad, d_pairs, the solver's best_s / best_R / best_t as d_s12 /
 * d_R12 / d_t12, and its d_matches12 rows as io->matches12, nothing copied or re-indexed in between.  `in`: kps (pt, octave), counts, img_stride, Tcw,
 * mp_world, mp_valid (NULL: every feature holds a point) and fx, fy, cx, cy are read (K1 = K2); mvInvLevelSigma2 is the context's.  matches12
 * [n_pairs][capacity], in / out: value v at i < N1 is a correspondence iff 0 <= v < N2 (-1, -2 and >= N2 are "none" and stay as they are), both features
 * hold a point and neither point is bad (:2068-2103; an entry that fails these keeps its value and is counted nowhere); an outlier of either check
 * becomes -1.  d_row_active (or NULL: every pair runs) [n_pairs]: olf_sim3_solver_io.accepted.  th2 > 0 (the reference: 10); fix_scale: bFixScale.
 * Per pair: S12_out [8] doubles (the quaternion as x, y, z, w -- g2o does not normalise it --, t, s) with its float forms s12_out, R12_out [9] (row-major,
 * toRotationMatrix), t12_out [3], which olf_search_by_sim3_pairs_dev or another round takes; Scw_out [16] = toCvMat(gScm * Sim3(R2w, t2w, 1.0))
 * (src/LoopClosing.cc:339-341), row-major, the d_Scw of olf_search_by_projection_sim3_batch_dev; n_inliers, the return value (0 where the `< 10` gate
 * returned: the matches are nulled and S12_out is the input; -1 for an inactive or refused pair, of which nothing else is written); n_correspondences;
 * n_bad_first (nBad); iters [2], the Levenberg iterations of the two optimize() calls; status, the pair's own word; chi2 [capacity][2], the values
 * (e12, e21) each correspondence was last classified with, 0 elsewhere.
 * Defined here, not by the reference: a depth of exactly 0 at any evaluation, the perturbed ones included (status bit 1), or an H, b, step or estimate that
 * is not finite (bit 2) stops the pair: S12_out is the input, the match row as it stood at that moment, n_inliers = 0.  An empty graph returns 0.  A
 * correspondence either of whose octaves lies outside the context's levels is left out and sets bit 4.  A pair whose index lies outside [0, n_frames), or
 * with kf1 == kf2, sets bit 2048 of the context's status word.
 * One launch: one workgroup per pair (grid-strided above 1024 pairs); the sums have a fixed correspondence-to-lane assignment and a fixed reduction shape,
 * so a pair's outputs are the same bits wherever it stands in the list.  The device's exp / sin / cos are not the host's, and the numeric Jacobian
 * amplifies a last-bit difference: device and host form agree on the real outputs within the tolerance the tests state, not bit for bit.  Like the other
 * batch entries: no synchronisation and no host read, the batch scratch slot (only where 69 bytes per feature of the capacity exceed 60 KiB of LDS: that
 * much per resident workgroup), n_pairs == 0 writes nothing, a NULL required pointer or th2 <= 0 is OLF_ERR_INVALID before any launch, a count beyond the
 * capacity is read as the capacity, accesses are never out of bounds. */
typedef struct olf_optimize_sim3_io {
    int32_t* matches12;          /* [n_pairs][capacity]     in / out */
    double*  S12_out;            /* [n_pairs][8]  */
    float*   s12_out;            /* [n_pairs]     */
    float*   R12_out;            /* [n_pairs][9]  */
    float*   t12_out;            /* [n_pairs][3]  */
    float*   Scw_out;            /* [n_pairs][16] */
    int32_t* n_inliers;          /* [n_pairs]     */
    int32_t* n_correspondences;  /* [n_pairs]     */
    int32_t* n_bad_first;        /* [n_pairs]     */
    int32_t* iters;              /* [n_pairs][2]  */
    int32_t* status;             /* [n_pairs]     */
    float*   chi2;               /* [n_pairs][capacity][2] */
} olf_optimize_sim3_io;
int olf_optimize_sim3_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                                const float* d_s12, const float* d_R12, const float* d_t12, float th2, int fix_scale, const int32_t* d_row_active,
                                const olf_optimize_sim3_io* io, void* stream);
/* the host form: ONE pair (kf1, kf2), host pointers in `in` and everywhere else, no context and no device, every sum serial in edge order.  capacity: the
 * row length of the per-frame planes; inv_level_sigma2 [n_levels] = mvInvLevelSigma2; every pointer of io names this pair's element or row; without a
 * context bit 2048 goes into the pair's status word. */
int olf_optimize_sim3(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* inv_level_sigma2, int n_levels, int kf1,
                      int kf2, float s12, const float* R12, const float* t12, float th2, int fix_scale, const olf_optimize_sim3_io* io);
/* olf_optimize_sim3_pairs_dev from host pointers ON THE DEVICE (csrc/optsim3_api.cpp): the arrays are staged (the in / out rows and the outputs are
 * uploaded first, so what the kernel leaves untouched comes back as it went in), the same kernel runs on the context's stream, the outputs come back;
 * synchronises.  A set bit of the context's status word makes the call return OLF_ERR_CAPACITY with the bit's text, the outputs complete. */
int olf_optimize_sim3_pairs(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* mp_bad, int n_pairs, const int32_t* pairs, const float* s12,
                            const float* R12, const float* t12, float th2, int fix_scale, const int32_t* row_active, const olf_optimize_sim3_io* io);
/* tests: the LDS a workgroup may take for a pair's correspondences (bytes; above it they live in context scratch; <= 0 restores the default), and the
 * numeric Jacobian of one edge (base_binary_edge.hpp:176-200) at an estimate: S12 [8] as S12_out, cam = fx, fy, cx, cy, X [3] the fixed point (P2c, or
 * P1c with inverse != 0 for the inverse edge), obs [2], J [2][7] row-major; a depth of exactly 0 is OLF_ERR_INVALID */
int olf_debug_optimize_sim3_lds_limit(int bytes);
int olf_debug_optimize_sim3_jacobian(const double* S12, int fix_scale, const double* cam, const double* X, const double* obs, int inverse, double* J);

/* ---- PnPsolver's RANSAC for a list of (key frame, frame) pairs on the device (csrc/pnpsolver_batch.hip) --------------------------------------------------
 * PnPsolver (src/PnPsolver.cc: EPnP inside a RANSAC) as Tracking::Relocalization drives it per candidate key frame (src/Tracking.cc:2255-2308): the
 * constructor's correspondences (:67-110), SetRansacParameters(probability, min_inliers, max_iterations, min_set, epsilon, th2) (:121-157; the tracker:
 * 0.99, 10, 300, 4, 0.5, 5.991) and one iterate(n_iterations, ...) per call (:165-258) with Refine (:260-305), for n_pairs pairs of the n_frames frames of
 * a batch.  It stands between olf_search_by_bow_pairs_dev (form OLF_BOW_KF_FRAME), whose rows it reads, and olf_search_by_projection_kf_pairs_dev, whose
 * d_Tcw takes Tcw; olf_pnp_apply_inliers_dev does :2297-2308 between them and olf_pose_optimization_batch_dev is Optimizer::PoseOptimization (:2310).  Results equal
 * olf_pnp_solver pair by pair, bit for bit, and do not depend on scheduling, on how the kernel chunks a window or on a pair's position in the list.
 * `in`: kps (pt of the frame's features, octave), counts, img_stride, mp_world and mp_valid of the key frame (NULL: every feature holds a point) and fx,
 * fy, cx, cy are read (frame j = image j * img_stride; a count beyond the capacity is read as the capacity); mvLevelSigma2 is the context's.  d_mp_bad
 * [n_frames][capacity] (or NULL: none is bad): isBad() of the point a feature holds.  d_pairs [n_pairs][2] = (key frame, frame), as the BoW form orders
 * them.  d_matches [n_pairs][capacity], read only: exactly the row olf_search_by_bow_pairs_dev writes; value v at frame feature i < N_frame is a
 * correspondence iff 0 <= v < N_kf (-1, -2 and >= N_kf are all "none"), key-frame feature v holds a point and that point is not bad: the 2-D point is
 * kps[i].pt, the 3-D point mp_world[kf][v], mvMaxError = sf * sf * th2 in float from the frame feature's octave.  Correspondences are kept in ascending i.
 * One whose octave lies outside the context's levels is left out and sets bit 256 of the context's status word.
 * olf_pnp_ransac: probability in (0, 1), min_inliers >= 1, max_iterations >= 1, min_set == 4, epsilon in (0, 1], th2 > 0, n_iterations >= 0: the window of
 * this call (the tracker: 5; max_iterations gives find()).  The effective min_inliers (max(N * epsilon truncated, min_inliers, min_set)) and the iteration
 * cap are functions of the number of correspondences alone; the call computes them for every N in [0, capacity] on the host with the host's libm
 * (csrc/pnpsolver_terms.hpp: pnp_parameters -- the exponent of epsilon is 3 as in the reference) and the kernel looks them up.
 * The loop condition of iterate (:182) is an OR: a call runs until the cap is reached AND n_iterations of its own are done, unless it accepts first; so
 * every call that does not accept ends with no_more = 1, and a call beyond the cap still runs n_iterations.
 * d_draws [n_pairs][max_iterations][4] (uint32): the raw rand() values below 2^31 of every iteration (convention C.20; bit 31 is ignored), indexed by
 * ABSOLUTE iteration modulo max_iterations (C.26), so a resumed call reads on where the last one stopped.
 * olf_pnp_solver_io, device pointers, one element or row per pair.  In and out -- the solver's carried state, all zero for a new solver: iterations_done
 * (mnIterations), best_inliers (mnBestInliers), best_Tcw [16] (mBestTcw, row-major), best_flags [capacity] (mvbBestInliers, uint8, by frame feature;
 * only features that are correspondences are written), and Refine's outcome for the current best set -- Refine is a function of that set alone, so it
 * runs when the best changes and is carried: refined_inliers (mnRefinedInliers), refined_Tcw [16], refined_flags [capacity].  An iteration with
 * n >= min_inliers and n > best_inliers replaces the best; the first iteration with n >= min_inliers whose best set's refined_inliers > min_inliers
 * (strict, :292) is accepted and ends the call -- so a solver that has accepted accepts again at the next such iteration (Tracking.cc:2312 `continue`).
 * Out: accepted (the returned pose is not empty: Refine accepted, or the cap was reached with best_inliers >= min_inliers, :241-255), no_more (bNoMore),
 * n_inliers (0 unless accepted), inliers [n_pairs][capacity] (uint8, by frame feature; positions below N_frame are written, all 0 unless accepted;
 * positions from N_frame on are left as they are), Tcw [16] (written only when accepted: refined_Tcw, or best_Tcw at the cap), n_correspondences (N), and
 * counts [n_pairs][max_iterations] (may be NULL): the inlier count of every iteration this call evaluated at its index modulo max_iterations, the others
 * untouched.  N < the effective min_inliers: no_more = 1 and the state is untouched.
 * Arithmetic (csrc/pnpsolver_terms.hpp and, for the sample of C.20, ransac_terms.hpp: one text for this entry and its host form; C.4, C.19, C.20,
 * C.23 to C.26 of DESIGN.md): compute_pose in double as written; the OpenCV calls as an OpenCV without LAPACK makes them (one-sided Jacobi in double; cvSolve / cvInvert skip singular values at or below
 * 2 DBL_EPSILON times their sum); qr_solve's singular return leaves x at 0 in the first Gauss-Newton round; sums over the correspondences in the
 * reference's order in a four-point fit and in a fixed blocked order in Refine (256 partial sums by index modulo 256, a balanced tree of neighbours per
 * 64, the four results in ascending order).  OpenCV's fill of a singular vector whose norm is <= DBL_MIN from its fixed-seed generator is NOT restated:
 * a hypothesis that would read such a vector (the PCA of the control points, M^t M, ABt) counts no inlier, a Refine that would fails, and bit 32768 of the
 * context's status word is set (the status text names the bit by number only).
 * A pair whose index lies outside [0, n_frames), or with both indices equal, gets n_inliers = -1, nothing else of it is written, and bit 2048 is set.
 * Errors, before any launch: a NULL required pointer, a negative count, min_set != 4, epsilon outside (0, 1], th2 <= 0, min_inliers < 1,
 * max_iterations < 1, n_iterations < 0 or probability outside (0, 1): OLF_ERR_INVALID.  n_pairs == 0 writes nothing.  Does not synchronise; runs on
 * `stream`.  Nothing is read or written out of bounds.
 * Scratch: 8 bytes per feature of the capacity (+ 8) and, where 32 bytes per feature of the capacity exceed the 46 KiB of LDS a workgroup has beside
 * its fit workspaces, that much per resident workgroup (at most 1024). */
typedef struct olf_pnp_ransac {
    double  probability;
    int32_t min_inliers, max_iterations, min_set, n_iterations;
    float   epsilon, th2;
} olf_pnp_ransac;
typedef struct olf_pnp_solver_io {
    int32_t* iterations_done;    /* [n_pairs]            in / out */
    int32_t* best_inliers;       /* [n_pairs]            in / out */
    float*   best_Tcw;           /* [n_pairs][16]        in / out */
    uint8_t* best_flags;         /* [n_pairs][capacity]  in / out */
    int32_t* refined_inliers;    /* [n_pairs]            in / out */
    float*   refined_Tcw;        /* [n_pairs][16]        in / out */
    uint8_t* refined_flags;      /* [n_pairs][capacity]  in / out */
    int32_t* accepted;           /* [n_pairs] */
    int32_t* no_more;            /* [n_pairs] */
    int32_t* n_inliers;          /* [n_pairs] */
    uint8_t* inliers;            /* [n_pairs][capacity] */
    float*   Tcw;                /* [n_pairs][16]: d_Tcw of olf_search_by_projection_kf_pairs_dev */
    int32_t* n_correspondences;  /* [n_pairs] */
    int32_t* counts;             /* [n_pairs][max_iterations], or NULL */
} olf_pnp_solver_io;
int olf_pnp_solver_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* d_mp_bad, int n_pairs, const int32_t* d_pairs,
                             const int32_t* d_matches, const olf_pnp_ransac* ransac, const uint32_t* d_draws, const olf_pnp_solver_io* io, void* stream);
/* Tracking.cc:2297-2308 for every pair with accepted > 0 (d_n_inliers < 0, a refused pair, or accepted <= 0: its rows stay as they are), for i in
 * [0, capacity): d_out[p][i] = d_matches[p][i] where d_inliers[p][i] is set and i < N_frame, -1 elsewhere (d_out may be d_matches itself);
 * d_cur_valid[p][i] = 1 / 0 likewise; d_already_found[p][v] = 1 for every such inlier's key-frame feature v, 0 elsewhere.  These are d_cur_valid and
 * d_already_found of olf_search_by_projection_kf_pairs_dev, whose pairs are ordered (current frame, key frame).  Any of the three outputs may be NULL.
 * `in`: counts and img_stride are read.  Does not synchronise. */
int olf_pnp_apply_inliers_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const uint8_t* d_inliers, const int32_t* d_accepted, const int32_t* d_n_inliers, int32_t* d_out, uint8_t* d_cur_valid,
                              uint8_t* d_already_found, void* stream);
/* the host form: ONE pair (kf, frame), host pointers in `in` and everywhere else, no context and no device, the loop of PnPsolver::iterate.  capacity: the
 * row length of the per-frame planes; scale_factors [n_levels] = mvScaleFactors; matches [capacity], draws [max_iterations][4]; every pointer of io names
 * this pair's element or row; *status receives the bits 256 / 2048 / 32768. */
int olf_pnp_solver(const olf_track_batch* in, int capacity, int n_frames, const uint8_t* mp_bad, const float* scale_factors, int n_levels, int kf, int frame,
                   const int32_t* matches, const olf_pnp_ransac* ransac, const uint32_t* draws, const olf_pnp_solver_io* io, int32_t* status);
/* olf_pnp_solver_pairs_dev from host pointers ON THE DEVICE (csrc/pnpsolver_api.cpp): the arrays are staged (the in / out state and the outputs are
 * uploaded first), the same kernel runs on the context's stream, state and outputs come back; synchronises.  A set status bit makes the call return
 * OLF_ERR_CAPACITY, the outputs complete. */
int olf_pnp_solver_pairs(olf_ctx* ctx, const olf_track_batch* in, int n_frames, const uint8_t* mp_bad, int n_pairs, const int32_t* pairs,
                         const int32_t* matches, const olf_pnp_ransac* ransac, const uint32_t* draws, const olf_pnp_solver_io* io);
/* tests: the LDS a workgroup of the solver may take for its correspondences (bytes; above it they live in context scratch; <= 0 restores the default),
 * and the parameters the solver's table holds for N correspondences (csrc/pnpsolver_terms.hpp: pnp_parameters) */
int olf_debug_pnp_solver_lds_limit(int bytes);
int olf_debug_pnp_solver_parameters(int N, const olf_pnp_ransac* ransac, int32_t* min_inliers, int32_t* cap);

/* ---- Initializer::Initialize for a list of frame pairs on the device (csrc/initializer_batch.hip) --------------------------------------------------------
 * Initializer (src/Initializer.cc: the homography / fundamental-matrix RANSAC with model selection and two-view reconstruction) as
 * Tracking::MonocularInitialization drives it (src/Tracking.cc:722 `new Initializer(frame, 1.0, 200)`, :756 `Initialize(...)`): Initialize (:44-121) with
 * FindHomography, FindFundamental, ComputeH21, ComputeF21, CheckHomography, CheckFundamental, Normalize, ReconstructF, ReconstructH, DecomposeE, CheckRT
 * and Triangulate, for n_pairs pairs of the n_frames frames of a batch.  It stands behind olf_search_for_initialization, whose rows it reads as they
 * are; olf_initializer_apply_dev does :758-772 behind it.  Results equal olf_initializer pair by pair, bit for bit, and do not depend on scheduling, on a
 * pair's position in the list or on where a pair's correspondences live.
 * `in`: kps (pt of mvKeysUn), counts, img_stride and fx, fy, cx, cy are read (frame j = image j * img_stride; a count beyond the capacity is read as the
 * capacity).  d_pairs [n_pairs][2] = (reference frame 1, current frame 2).  d_matches [n_pairs][capacity], read only: exactly the vnMatches12 row
 * olf_search_for_initialization writes; value v at reference feature i < N1 is a correspondence iff 0 <= v < N2.  Correspondences are kept in ascending
 * i: mvMatches12.  Normalize runs over ALL key points of each frame, as written.
 * olf_initializer_params: sigma (> 0), max_iterations (>= 1), min_parallax (degrees, finite), min_triangulated (>= 0); the tracker: 1.0, 200, 1.0, 50.
 * d_draws [n_pairs][max_iterations][8] (uint32): the raw rand() values of every iteration's eight draws (convention C.20; bit 31 is ignored); both
 * RANSACs read the same sets (mvSets).  The reference's SeedRandOnce(0) + rand() stream is the caller's business (InitializerOf,
 * include/orbline_reference_api.hpp).
 * olf_initializer_io, device pointers, one element or row per pair, all outputs (Initialize carries no state): ok (the return value; -1: a refused
 * pair), n_correspondences (N), model (0: none was evaluated, 1: H was reconstructed, 2: F), score_H, score_F, H21 [9], F21 [9] (the best of each
 * RANSAC, row-major; left untouched when no iteration scored above 0), inliers_H, inliers_F [capacity] (uint8 by reference feature; positions below N1
 * are written, positions from N1 on are left as they are), R21 [9], t21 [3] (written only when ok), P3D [capacity][3] and triangulated [capacity] (vP3D
 * and vbTriangulated of the chosen hypothesis, written below N1 only when ok; entries CheckRT did not assign are the zeros of resize), n_good [8]
 * (nGood of every hypothesis evaluated, 4 for F and 8 for H; the others 0), cos_parallax [8] (vCosParallax[min(50, n - 1)] of each, 0 where
 * nGood == 0 -- the COSINE, not degrees: parallax = acos(c) * 180 / pi is formed by the caller on the host, as the Python wrapper and the adaptor
 * do), hypothesis (the chosen index, or -1).  N < 8 (undefined in the reference, which draws from an empty list): ok = 0, model = 0, and beside them
 * only n_correspondences is written.  With N >= 8 everything but H21 / F21 / R21 / t21 / P3D / triangulated is written.
 * Arithmetic (csrc/initializer_terms.hpp and, for the sample of C.20, ransac_terms.hpp: one text for this entry and its host form; C.4, C.12, C.17 to
 * C.20, C.30 to C.35 of DESIGN.md): cv::SVDecomp as an OpenCV without LAPACK makes it at 16 x 9, 8 x 9, 3 x 3 (C.30) and 4 x 4 (C.19, the text of
 * olf_create_new_map_points); the fundamental matrix's null vector is the row OpenCV fills for a zero singular value from its fixed-seed generator
 * (C.31, restated from memory and UNVERIFIED; at most 4 attempts, then the hypothesis is degenerate: it scores 0 and bit 32768 of the context's status
 * word is set, as for one of the eight rows at norm <= FLT_MIN); scores are summed sequentially in float in ascending reference feature and the first of
 * the maxima wins (C.32); no acos on the device: the entry finds, on the host with the host's libm, the float cosine thresholds equivalent to
 * `parallax > min_parallax` (ReconstructF) and `parallax >= min_parallax` (ReconstructH) and the kernel compares cosines (C.34); the 51st cosine is a
 * selection with NaN last, and a NaN among a hypothesis' good cosines sets bit 65536 (C.35).
 * A pair whose index lies outside [0, n_frames), or with both indices equal, gets ok = -1, nothing else of it is written, and bit 2048 is set.
 * Errors, before any launch: a NULL required pointer, a negative count, sigma <= 0, max_iterations < 1, min_triangulated < 0 or a parameter that is not
 * finite: OLF_ERR_INVALID.  n_pairs == 0 writes nothing.  Does not synchronise; runs on `stream`.  Nothing is read or written out of bounds.
 * Scratch: where 32 bytes per feature of the capacity exceed the 24 KiB of LDS a workgroup has beside its fit workspaces, that much per resident
 * workgroup (at most 1024). */
typedef struct olf_initializer_params {
    float   sigma;
    int32_t max_iterations;
    float   min_parallax;
    int32_t min_triangulated;
} olf_initializer_params;
typedef struct olf_initializer_io {
    int32_t* ok;                 /* [n_pairs] */
    int32_t* n_correspondences;  /* [n_pairs] */
    int32_t* model;              /* [n_pairs] */
    float*   score_H;            /* [n_pairs] */
    float*   score_F;            /* [n_pairs] */
    float*   H21;                /* [n_pairs][9] */
    float*   F21;                /* [n_pairs][9] */
    uint8_t* inliers_H;          /* [n_pairs][capacity] */
    uint8_t* inliers_F;          /* [n_pairs][capacity] */
    float*   R21;                /* [n_pairs][9] */
    float*   t21;                /* [n_pairs][3] */
    float*   P3D;                /* [n_pairs][capacity][3] */
    uint8_t* triangulated;       /* [n_pairs][capacity] */
    int32_t* n_good;             /* [n_pairs][8] */
    float*   cos_parallax;       /* [n_pairs][8] */
    int32_t* hypothesis;         /* [n_pairs] */
} olf_initializer_io;
int olf_initializer_pairs_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const olf_initializer_params* params, const uint32_t* d_draws, const olf_initializer_io* io, void* stream);
/* Tracking.cc:758-772 for every pair with d_ok > 0 (the rows of the others stay as they are), for i in [0, capacity): d_out[p][i] = d_matches[p][i]
 * where i < N1, the value is a correspondence and d_triangulated[p][i] is set, -1 elsewhere (d_out may be d_matches itself); d_n_matches[p]: how many
 * remain; d_Tcw [n_pairs][16]: the current frame's pose, eye(4, 4) with d_R21 and d_t21 copied in (the reference frame's is the identity).  Any of the
 * three outputs may be NULL.  `in`: counts and img_stride are read.  Does not synchronise. */
int olf_initializer_apply_dev(olf_ctx* ctx, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* d_pairs, const int32_t* d_matches,
                              const uint8_t* d_triangulated, const int32_t* d_ok, const float* d_R21, const float* d_t21, int32_t* d_out,
                              int32_t* d_n_matches, float* d_Tcw, void* stream);
/* the host form: ONE pair (ref, cur), host pointers in `in` and everywhere else, no context and no device.  capacity: the row length of the per-frame
 * planes; matches [capacity], draws [max_iterations][8]; every pointer of io names this pair's element or row; *status receives the bits 2048 / 32768 /
 * 65536. */
int olf_initializer(const olf_track_batch* in, int capacity, int n_frames, int ref, int cur, const int32_t* matches, const olf_initializer_params* params,
                    const uint32_t* draws, const olf_initializer_io* io, int32_t* status);
/* olf_initializer_pairs_dev from host pointers ON THE DEVICE (csrc/initializer_api.cpp): the arrays are staged (the outputs are uploaded first, so what
 * the device leaves untouched comes back as it went in), the same kernel runs on the context's stream, the outputs come back; synchronises.  A set
 * status bit makes the call return OLF_ERR_CAPACITY, the outputs complete. */
int olf_initializer_pairs(olf_ctx* ctx, const olf_track_batch* in, int n_frames, int n_pairs, const int32_t* pairs, const int32_t* matches,
                          const olf_initializer_params* params, const uint32_t* draws, const olf_initializer_io* io);
/* tests: the LDS a workgroup of the initialiser may take for its correspondences (bytes; above it they live in context scratch; <= 0 restores the
 * default), and C.34's two cosine thresholds for a min_parallax as this machine's acosf gives them (NaN: no cosine passes) */
int olf_debug_initializer_lds_limit(int bytes);
int olf_debug_initializer_cos_thresholds(float min_parallax, float* cos_gt, float* cos_ge);
/* tests: the eight sample indices ransac_sample<8> (csrc/ransac_terms.hpp) makes of eight draws among N >= 8 correspondences */
int olf_debug_initializer_sample(int N, const uint32_t* draws8, int32_t* idx8);

/* measurement: rate of a plain 16-byte-per-thread device copy kernel over `bytes` (read + written bytes per second): the practical HBM
 * ceiling bench.py reports next to the specification's 8 TB/s */
int olf_debug_copy_bandwidth(olf_ctx* ctx, size_t bytes, int reps, double* gbytes_per_s);

/* ---- place recognition: KeyFrameDatabase (src/KeyFrameDatabase.cc) and TemplatedVocabulary::score with L1 scoring -------------------------------
 * A database holds the BoW vectors of its key frames for the point and (optionally) the line vocabulary.  A key frame is a SLOT: olf_kfdb_add hands out
 * 0, 1, 2, ... in the order of the add calls, a slot is never reused until olf_kfdb_clear and an erased slot stays as an empty column of the tables.  The
 * slot order stands for two orders of the reference: the insertion order of a word's posting list (mvInvertedFile[w].push_back, :51-54) and the address
 * order of the std::set the WithLine forms iterate (:307, :582; DESIGN 2, convention C.15).
 * The data-parallel part (common-word counts, smallest common word and L1 scores of Q queries against every slot) runs on the device; the sequential,
 * stateful part (thresholds, covisibility accumulation, the per-key-frame members mRelocScore / mRelocScore_l / mRelocScore_pl that survive a query) is
 * host code behind olf_kfdb_select.
 * Limits (OLF_ERR_CAPACITY, checked before anything is launched): OLF_KFDB_MAX_WORDS words per BoW vector, OLF_KFDB_MAX_SLOTS slots,
 * OLF_KFDB_MAX_CELLS = Q x slots table entries per call, 2^31 - 1 words in a database per vocabulary. */
#define OLF_KFDB_MAX_WORDS 4096
#define OLF_KFDB_MAX_SLOTS (1 << 20)
#define OLF_KFDB_MAX_CELLS (1 << 26)
#define OLF_SCORING_L1_NORM 0                  /* DBoW2::ScoringType, Thirdparty/DBoW2/DBoW2/BowVector.h:45-53 */
#define OLF_KFDB_LOOP            0             /* DetectLoopCandidates                    src/KeyFrameDatabase.cc:107-228 */
#define OLF_KFDB_LOOP_LINE       1             /* DetectLoopCandidatesWithLine            :230-400 */
#define OLF_KFDB_RELOC           2             /* DetectRelocalizationCandidates          :402-512 */
#define OLF_KFDB_RELOC_LINE      3             /* DetectRelocalizationCandidatesWithLine  :514-667 */
typedef struct olf_kfdb olf_kfdb;
/* n BoW vectors as CSR: vector i is ids / vals [off[i], off[i + 1]), ids ascending and distinct (a DBoW2::BowVector is a std::map) */
typedef struct olf_bow_csr { const int32_t* off; const int32_t* ids; const double* vals; } olf_bow_csr;
/* one vocabulary's tables, [n_queries][n_slots] row-major: common = number of common words (mnLoopWords / mnRelocWords as the walk :117-135 leaves them
 * for a key frame that is not connected), first = the smallest common word id or -1 (the walk's first encounter), score = L1Scoring::score(query, slot)
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) bit for bit where common > 0 and -0.0 elsewhere */
typedef struct olf_kfdb_tables { int32_t* common; int32_t* first; double* score; } olf_kfdb_tables;

/* KeyFrameDatabase::KeyFrameDatabase (:33-44).  n_words_p / n_words_l: the vocabularies' sizes; n_words_l == 0: no line vocabulary, the WithLine forms
 * return empty lists (:232, :516).  A scoring other than OLF_SCORING_L1_NORM (what both of the reference's vocabularies use): OLF_ERR_INVALID.  ctx may be
 * NULL: such a database keeps no device copy and serves add / erase / clear / size / select / state only. */
int olf_kfdb_create(olf_ctx* ctx, int n_words_p, int n_words_l, int scoring_p, int scoring_l, olf_kfdb** out);
void olf_kfdb_destroy(olf_kfdb* db);
/* KeyFrameDatabase::add (:46-55): the key frame's mBowVec and mBowVec_l as host arrays (ids ascending, distinct, in [0, n_words)); *slot: its slot.
 * Must not overlap a tables call of the same database that is still running (the device arrays may move). */
int olf_kfdb_add(olf_kfdb* db, const int32_t* ids_p, const double* vals_p, int n_p, const int32_t* ids_l, const double* vals_l, int n_l, int32_t* slot);
/* KeyFrameDatabase::erase (:57-90): the slot becomes an empty column.  Erasing an erased slot is a no-op; the per-slot state stays (it is the key frame's). */
int olf_kfdb_erase(olf_kfdb* db, int32_t slot);
/* KeyFrameDatabase::clear (:92-98); the slot numbers start again at 0, the per-slot state and the query id bounds are reset */
int olf_kfdb_clear(olf_kfdb* db);
/* *n_slots: slots handed out since the last clear (the row length of the tables); *n_live: those not erased */
int olf_kfdb_size(const olf_kfdb* db, int32_t* n_slots, int32_t* n_live);
/* the members that survive a query, [n_slots] each (NULL: not wanted): mRelocScore, mRelocScore_l, mRelocScore_pl; 0 until written (src/KeyFrame.cc:35-37) */
int olf_kfdb_state(const olf_kfdb* db, float* reloc_score, float* reloc_score_l, float* reloc_score_pl);
/* The walks :117-135, :246-284, :410-425, :528-560 without the connected-key-frame test, and mpVoc->score (:164, :334-335, :452, :605-606), for n_queries
 * queries against every slot.  qp / ql: the queries' mBowVec / mBowVec_l; off are HOST arrays [n_queries + 1] (the limits are checked from them), ids and
 * vals device arrays.  d_tp / d_tl: device tables [n_queries][n_slots].  ql and d_tl may be NULL (both or neither): the line tables are not computed.
 * Enqueued on `stream` (NULL: the context's own); no synchronise. */
int olf_kfdb_tables_dev(olf_kfdb* db, int n_queries, const olf_bow_csr* qp, const olf_bow_csr* ql, const olf_kfdb_tables* d_tp, const olf_kfdb_tables* d_tl,
                        void* stream);
/* The rest of the four Detect members for n_queries queries, one after the other in list order (query q + 1 sees the state query q left).  Host only.
 * form: OLF_KFDB_*.  query_ids: pKF->mnId / F->mnId, > 0 and strictly greater than any id an earlier query of the same family (loop, relocalisation) of
 * this database had, else OLF_ERR_INVALID with nothing changed.  np, nl [n_queries]: N and N_l (WithLine forms; else NULL).  min_score [n_queries]
 * (loop forms; else NULL).  conn_off [n_queries + 1] / conn_slots: GetConnectedKeyFrames() of each query as slots (loop forms; NULL: none; values
 * outside [0, n_slots) are key frames outside the database and ignored).  nb_off [n_slots + 1] / nb_slots: GetBestCovisibilityKeyFrames(10) of every
 * slot in order, a negative value = a neighbour that is not in the database (skipped); values >= n_slots: OLF_ERR_INVALID.  n_slots must be the
 * database's.  tp, tl: host copies of the tables (tl NULL in the plain forms).  Out: cand_off [n_queries + 1] and cand_slots [cand_capacity], the
 * candidates of each query in the reference's order; more than cand_capacity candidates: OLF_ERR_CAPACITY with nothing changed. */
int olf_kfdb_select(olf_kfdb* db, int form, int n_queries, const int64_t* query_ids, const int32_t* np, const int32_t* nl, const float* min_score,
                    const int32_t* conn_off, const int32_t* conn_slots, const int32_t* nb_off, const int32_t* nb_slots, int n_slots,
                    const olf_kfdb_tables* tp, const olf_kfdb_tables* tl, int32_t* cand_off, int32_t* cand_slots, int cand_capacity);
/* tables, download, select: every pointer a host pointer (qp->off included); the arguments of the two entries above */
int olf_kfdb_detect(olf_kfdb* db, int form, int n_queries, const int64_t* query_ids, const olf_bow_csr* qp, const olf_bow_csr* ql, const int32_t* np,
                    const int32_t* nl, const float* min_score, const int32_t* conn_off, const int32_t* conn_slots, const int32_t* nb_off,
                    const int32_t* nb_slots, int32_t* cand_off, int32_t* cand_slots, int cand_capacity);
/* The minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:126-144): d_score[i] = L1Scoring::score(a_i, b_i) for n_pairs pairs d_pairs [n_pairs][2]
 * (device).  b_i is a slot of the database's vocabulary `line` (0 points, 1 lines); a_i is a slot too when d_queries is NULL, else vector a_i of the
 * n_queries device vectors d_queries (off a DEVICE array here).  A pair with an index out of range scores NaN. */
int olf_bow_score_pairs_dev(olf_kfdb* db, int line, int n_pairs, const int32_t* d_pairs, const olf_bow_csr* d_queries, int n_queries, double* d_score,
                            void* stream);
/* TemplatedVocabulary::score (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1199-1203) with L1 scoring for two host vectors, on the device */
int olf_bow_score(olf_ctx* ctx, const int32_t* ids_a, const double* vals_a, int n_a, const int32_t* ids_b, const double* vals_b, int n_b, double* score);

/* ---- Optimizer::PoseOptimizationWithLine for a batch of frames on the device (csrc/pose_batch.hip, pose_host.cpp, pose_terms.hpp) -----------------------
 * bool Optimizer::PoseOptimizationWithLine(Frame*) (src/Optimizer.cc:604-777): the branch that executes (`if(true)`, :664-697), i.e. the point-and-line
 * Gauss-Newton solver of StVO-PL -- gaussNewtonOptimization twice, gaussNewtonOptimizationRobust, gaussNewtonOptimization, each from the same prior DT and
 * each followed by removeOutliers -- and its epilogue; the call of Tracking::TrackReferenceKeyFrameWithLine (src/Tracking.cc:1032),
 * TrackWithMotionModelWithLine (:1470) and TrackLocalMap (:1544).  Optimizer::PoseOptimization (g2o, points only) is olf_pose_optimization* below.  Doubles throughout, as the
 * reference; the arithmetic of every term is csrc/pose_terms.hpp, the same text for the host form and the kernel.  Defaults: src/Config.cpp:42-82. */
typedef struct olf_pose_params {
    int32_t max_iters_ref;       /* Config::maxItersRef()       10   (>= 1)                                          */
    double  homog_th;            /* Config::homogTh()           1e-7 (> 0)                                           */
    double  min_error;           /* Config::minError()          1e-7                                                 */
    double  min_error_change;    /* Config::minErrorChange()    1e-7                                                 */
    double  inlier_k;            /* Config::inlierK()           4.0                                                  */
    int32_t use_motion_model;    /* Config::useMotionModel()    1: DT = Tcw * inverse(Tcw_prev); 0: the identity     */
    int32_t has_points;          /* Config::hasPoints()         1; as in the reference it gates removeOutliers only: */
                                 /* with 0 the points still enter the sums, and their outlier flags on entry stay in  */
                                 /* force through all four passes (none is set, none is cleared); has_lines likewise  */
    int32_t has_lines;           /* Config::hasLines()          1                                                    */
} olf_pose_params;
void olf_pose_default_params(olf_pose_params* p);
/* The frames of a batch as the optimiser reads them.  Device pointers; frame j = image j * img_stride of the extractor-layout arrays kps / counts / kls /
 * lcounts (as olf_track_batch and olf_line_batch); every other plane is per frame, [n_frames][olf_orb_capacity()] or [n_frames][olf_line_capacity()].
 * A count beyond the capacity is read as the capacity.  mvInvLevelSigma2 is the context's; a line reads it by its key line's octave. */
typedef struct olf_pose_batch {
    const olf_keypoint* kps; const int32_t* counts;       /* mvKeysUn, N                                                                           */
    const olf_keyline* kls; const int32_t* lcounts;       /* mvKeysUn_Line, N_l                                                                    */
    int32_t img_stride;
    const double*  lle;               /* [n_frames][line capacity][3] mvle_l (olf_frame_buffers.lle)                                               */
    const float*   Tcw;               /* [n_frames][16] mTcw, row-major: the prior                                                                 */
    const float*   Tcw_prev;          /* [n_frames][16] mTcw_prev; NULL: empty, i.e. Tcw (:613-614)                                                */
    const double*  DT_cov_in;         /* [n_frames][36] pFrame->DT_cov on entry; NULL: zeros.  It is what DT_cov stays when a pass returns early (:790-795), */
                                      /* also with use_motion_model = 0, where the reference never loads it and leaves DT_cov uninitialised         */
    float fx, fy, cx, cy;
    const int32_t* frame_mp;          /* [n_frames][capacity] mvpMapPoints as indices into mp_world, negative = NULL                               */
    const int32_t* mp_index_offset;   /* [n_frames] added to every non-negative entry of the frame, or NULL.  The frame-to-frame searches return    */
                                      /* indices into the LAST frame's features: with mp_world = olf_track_batch.mp_world viewed flat and offset  */
                                      /* j * capacity for the pair's last frame j their output goes in as it is; map indices pass NULL             */
    const float*   mp_world;          /* [n_mp][3] GetWorldPos()                                                                                   */
    int32_t        n_mp;
    const int32_t* frame_ml;          /* [n_frames][line capacity], ml_index_offset [n_frames] or NULL, ml_world [n_ml][6] (olf_local_line_map.world). */
                                      /* olf_track_lines_batch_dev is NOT like the point search: its d_cur_ml holds the ids the caller gave the last */
                                      /* frame's lines (d_last_ml), not indices into the last frame.  With map indices as those ids d_cur_ml goes in  */
                                      /* as it is with ml_index_offset NULL; so does the output of olf_search_local_lines_batch_dev                  */
    const int32_t* ml_index_offset;
    const float*   ml_world;
    int32_t        n_ml;
    const uint8_t* outlier;           /* [n_frames][capacity] mvbOutlier on entry; NULL: none                                                      */
    const uint8_t* outlier_l;         /* [n_frames][line capacity] mvbOutlier_Line on entry; NULL: none                                            */
} olf_pose_batch;
/* What a call writes per frame.  Every pointer is required. */
typedef struct olf_pose_outputs {
    float*   Tcw_out;         /* [16]  the pose SetPose receives (:688-689)                                                                        */
    double*  DT;              /* [16]  pFrame->DT (:684)                                                                                            */
    double*  DT_cov;          /* [36]  pFrame->DT_cov                                                                                               */
    double*  DT_cov_eig;      /* [6]   pFrame->DT_cov_eig, ascending                                                                                */
    double*  err_norm;        /*       pFrame->err_norm                                                                                             */
    uint8_t* good;            /*       isGoodSolution(DT, DT_cov, err) (:453-466, :683), which the reference computes and ignores                   */
    uint8_t* outlier_out;     /* [capacity]      mvbOutlier at the end, 0 from the count on and for a feature that holds nothing; may be `outlier`  */
    uint8_t* outlier_l_out;   /* [line capacity] mvbOutlier_Line likewise; may be `outlier_l`                                                       */
    int32_t* n_inliers;       /* [2]   held and not outlier: points, lines (n_inliers_pt, n_inliers_ls)                                             */
    int32_t* iters;           /* [4]   evaluations of each pass, for diagnosis                                                                      */
    int32_t* status;          /*       the frame's own status word: 1, 2, 4 below                                                                   */
} olf_pose_outputs;
/* One launch for the whole batch: one workgroup per frame carries it through the four passes and the epilogue.  The 28 sums of an evaluation (H's upper
 * triangle, g, e) have a fixed feature-to-lane assignment and a fixed reduction shape, and the medians of vector_mean_stdv_mad / vector_stdv_mad
 * (src/Auxiliar.cc:399-472) are exact selections of element n / 2, so a frame's outputs are the same bits wherever it stands in a batch.
 *
 * Three things the reference leaves undefined are defined here:
 *  - a feature that enters with its outlier flag set: its previous-frame position is computed like any other (the reference reads a stale vector there;
 *    none of its call sites produces such a feature);
 *  - DT_cov when use_motion_model = 0 and a pass returns early: the reference's is uninitialised there, the entry's is DT_cov_in (or zeros);
 *  - a pass that starts with no active (held, not outlier) feature, or an H, g or DT that is not finite (the reference divides by zero): the frame stops
 *    there.  Its pose goes through unchanged (Tcw_out = Tcw), DT = I, DT_cov = 0, err_norm = -1, the eigenvalues 0, good = 0, its outlier flags stay as
 *    they stood, and bit 1 (no active feature) or bit 2 (not finite) of the frame's status word is set.
 * A held feature whose octave is outside the context's levels is left out (it holds nothing) and sets bit 4 of the frame's status word; an index at or past
 * n_mp / n_ml counts as "holds nothing" and sets bit 512 / 1024 of the context's status word.  Like the other batch entries: no synchronisation and no host
 * read, the batch scratch slot, n_frames == 0 writes nothing, a NULL required pointer is OLF_ERR_INVALID, accesses are never out of bounds. */
int olf_pose_optimization_with_line_batch_dev(olf_ctx* ctx, const olf_pose_batch* in, int n_frames, const olf_pose_params* params, const olf_pose_outputs* out,
                                              void* stream);
/* The host form: one frame (frame 0 of `in`), host pointers, no context and no device; plain doubles, every sum in the reference's index order.  capacity /
 * line_capacity: the lengths of the per-feature rows; inv_level_sigma2 [n_levels]: mvInvLevelSigma2 (olf_orb_scale_tables).  Without a context the bits
 * 512 / 1024 go into the frame's status word. */
int olf_pose_optimization_with_line(const olf_pose_batch* in, int capacity, int line_capacity, const float* inv_level_sigma2, int n_levels,
                                    const olf_pose_params* params, const olf_pose_outputs* out);
/* One frame from host pointers on the device: the rows of `in` (lengths counts[0] / lcounts[0], at most the context's capacities, else OLF_ERR_CAPACITY) are
 * staged, the batched kernel runs on a batch of one, the outputs come back (outlier_out [counts[0]], outlier_l_out [lcounts[0]]); synchronises.  An index
 * outside the maps makes the call return OLF_ERR_CAPACITY with the bit's text, the outputs complete. */
int olf_pose_optimization_with_line_frame(olf_ctx* ctx, const olf_pose_batch* in, const olf_pose_params* params, const olf_pose_outputs* out);
/* The "discard outliers" loops that follow the three calls, on the rows the optimiser read and wrote.  Device pointers, rows as above; frame_mp / frame_ml /
 * outlier / outlier_l are changed in place; mp_obs [n_mp] / ml_obs [n_ml]: Observations() > 0 (NULL: all).
 *  mode 0  src/Tracking.cc:1034-1074 (the same loops follow :1470): a held outlier is dropped (-1) and its flag cleared; n_matches = the held rest with
 *          Observations() > 0 (nmatchesMap_p, nmatchesMap_l);
 *  mode 1  :1547-1590: n_matches = held and not outlier, with Observations() > 0 unless only_tracking (mnMatchesInliers, mnMatchesInliers_l); a held outlier
 *          is dropped when `stereo` and keeps its flag.  IncreaseFound() stays the caller's: it is "held and not outlier" of the inputs.
 * d_n_matches [n_frames][2]: points, lines.  Indices at or past n_mp / n_ml are left alone and set bit 512 / 1024 of the context's status word. */
typedef struct olf_discard_batch {
    const int32_t* counts; const int32_t* lcounts; int32_t img_stride;
    int32_t* frame_mp; int32_t* frame_ml;
    uint8_t* outlier; uint8_t* outlier_l;
    const int32_t* mp_index_offset; const int32_t* ml_index_offset;
    const uint8_t* mp_obs; const uint8_t* ml_obs;
    int32_t n_mp, n_ml;
} olf_discard_batch;
int olf_discard_outliers_batch_dev(olf_ctx* ctx, const olf_discard_batch* io, int n_frames, int mode, int only_tracking, int stereo, int32_t* d_n_matches,
                                   void* stream);
/* one frame from host pointers on the device, as olf_pose_optimization_with_line_frame */
int olf_discard_outliers_frame(olf_ctx* ctx, const olf_discard_batch* io, int mode, int only_tracking, int stereo, int32_t* n_matches);
/* the host form: one frame, host pointers, no context; *status receives the bits 512 / 1024 */
int olf_discard_outliers(const olf_discard_batch* io, int capacity, int line_capacity, int mode, int only_tracking, int stereo, int32_t* n_matches,
                         int32_t* status);

/* ---- Optimizer::PoseOptimization for a list of rows on the device (csrc/posepoints_batch.hip, posepoints_host.cpp, posepoints_terms.hpp) --------------------
 * int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-451): the g2o graph of one free VertexSE3Expmap and one EdgeSE3ProjectXYZOnlyPose
 * (mvuRight[i] < 0) or EdgeStereoSE3ProjectXYZOnlyPose per held feature, in ascending feature index, Huber kernels with the float deltas sqrt(5.991) /
 * sqrt(7.815), four passes of OptimizationAlgorithmLevenberg (10 iterations, LinearSolverDense) each from toSE3Quat(mTcw), each followed by the chi2
 * classification in float, the kernels removed after the third, one pass only below 10 edges; the call of Tracking::Relocalization
 * (src/Tracking.cc:2310, :2326, :2341), TrackWithMotionModel (:1242 ff.) and TrackReferenceKeyFrame (:932 ff.).  Doubles throughout; the arithmetic of every
 * term is csrc/posepoints_terms.hpp, of Eigen's LDLT and of the Levenberg loop csrc/g2o_levenberg.hpp, the same text for the host form and the kernel (C.4, C.27).
 * A ROW is one call of the reference: relocalisation optimises one frame once per candidate key frame.  Device pointers.  Without `pairs`, row r reads
 * frame r (image r * img_stride of kps / counts, row r of uright) and a non-negative frame_mp value v is point v + mp_index_offset[r] of mp_world: the
 * convention of olf_pose_batch, so the output of the frame-to-frame and key-frame BoW searches goes in as documented there (n_rows <= n_frames).  With
 * `pairs` = (key frame, frame), the array olf_pnp_solver_pairs_dev takes, row r reads frame pairs[r][1]'s features and v is point
 * pairs[r][0] * capacity + v (+ mp_index_offset[r]) of olf_track_batch.mp_world viewed flat (n_mp = n_frames * capacity): Tcw is olf_pnp_solver_io.Tcw,
 * frame_mp is d_out of olf_pnp_apply_inliers_dev and row_active its d_accepted, nothing copied or re-indexed in between.  A row with row_active <= 0, or a
 * pair outside [0, n_frames) or with both indices equal (bit 2048 of the context's status word), gets n_good = -1 and nothing else of it is written.
 * There is no outlier input: the reference clears every held feature's flag on entry (:289, :323).
 * The stale-error quirk of the reference is kept: after a pass an edge whose flag is clear is classified with the _error the last computeActiveErrors()
 * left, which is the error at the REJECTED estimate when the pass's last Levenberg trial was rejected (pop() restores the vertex, not the edges).
 * Defined here, not by the reference: a held point at depth exactly 0 at an evaluation (status bit 1) or an H, b, step or estimate that is not finite
 * (bit 2) stops the row: Tcw_out = Tcw, the flags as they stood after the last completed pass, n_good = 0, `passes` the passes completed.  A pass whose
 * active set is empty leaves the estimate at toSE3Quat(mTcw) with iters = 0 and classifies every edge there (what g2o does: see posepoints_terms.hpp).  A
 * held feature whose octave is outside the context's levels holds nothing and sets bit 4 of the row's status; an index outside [0, n_mp) holds nothing and
 * sets bit 512 of the context's status word.
 * The loops that follow a call need no new entry: src/Tracking.cc:934-953 is olf_discard_outliers* mode 0 and :2315-2317 / :2343-2345 mode 1 with
 * stereo = 1 (dropped, flag kept) on frame_mp / outlier_out, without lines -- those entries want non-NULL line rows, so the caller passes an lcounts
 * array of zeros and any valid frame_ml / outlier_l pointers, which are then never read. */
typedef struct olf_pose_points_batch {
    const olf_keypoint* kps; const int32_t* counts; int32_t img_stride;   /* mvKeysUn (pt, octave), N                                         */
    const float*   uright;            /* [n_frames][capacity] mvuRight (olf_frame_buffers.uright); negative: a monocular edge               */
    float fx, fy, cx, cy, bf;         /* bf = mbf                                                                                            */
    const float*   Tcw;               /* [n_rows][16] mTcw, row-major                                                                        */
    const int32_t* frame_mp;          /* [n_rows][capacity] mvpMapPoints as indices, negative = NULL                                         */
    const float*   mp_world;          /* [n_mp][3] GetWorldPos()                                                                             */
    int32_t        n_mp;
    const int32_t* mp_index_offset;   /* [n_rows] or NULL                                                                                    */
    const int32_t* pairs;             /* [n_rows][2] (key frame, frame) or NULL                                                              */
    const int32_t* row_active;        /* [n_rows] or NULL: every row runs                                                                    */
} olf_pose_points_batch;
/* What a call writes per row.  Every pointer is required. */
typedef struct olf_pose_points_outputs {
    float*   Tcw_out;         /* [16]        the pose SetPose receives (:445-448)                                                              */
    uint8_t* outlier_out;     /* [capacity]  mvbOutlier at the end; 0 from the count on and where nothing is held                              */
    int32_t* n_good;          /*             the return value, nInitialCorrespondences - nBad of the last pass that ran; 0 below 3 edges       */
    int32_t* n_initial;       /*             nInitialCorrespondences                                                                           */
    float*   chi2;            /* [capacity]  the value each held feature was last classified with (0 elsewhere, and below 3 edges)             */
    int32_t* passes;          /*             passes completed (0 below 3 edges, 1 below 10)                                                    */
    int32_t* iters;           /* [4]         Levenberg iterations of each pass                                                                 */
    int32_t* status;          /*             the row's own status word: 1, 2, 4 above                                                          */
} olf_pose_points_outputs;
/* One launch: one workgroup per row (grid-strided above 1024 rows) carries it through the four passes; activeRobustChi2 and the 21 + 6 sums of
 * buildSystem have a fixed feature-to-lane assignment and a fixed reduction shape, so a row's outputs are the same bits wherever it stands in the list.
 * Like the other batch entries: no synchronisation and no host read, the batch scratch slot (only where 29 bytes per feature of the capacity exceed
 * 60 KiB of LDS: that much per resident workgroup), n_rows == 0 writes nothing, a NULL required pointer is OLF_ERR_INVALID, a count beyond the capacity is
 * read as the capacity, accesses are never out of bounds. */
int olf_pose_optimization_batch_dev(olf_ctx* ctx, const olf_pose_points_batch* in, int n_rows, int n_frames, const olf_pose_points_outputs* out, void* stream);
/* The host form: row 0 of `in`, host pointers, no context and no device; plain doubles, every sum in ascending feature index.  capacity: the length of
 * the per-feature rows; inv_level_sigma2 [n_levels]: mvInvLevelSigma2.  Without a context the bits 512 / 2048 go into the row's status word. */
int olf_pose_optimization(const olf_pose_points_batch* in, int capacity, int n_frames, const float* inv_level_sigma2, int n_levels,
                          const olf_pose_points_outputs* out);
/* olf_pose_optimization_batch_dev from host pointers (csrc/posepoints_api.cpp): every array at the context's capacity is staged (the outputs are uploaded
 * first, so an untouched row comes back as it went in), the kernel runs on the context's stream, the outputs come back; synchronises.  A set bit of the
 * context's status word makes the call return OLF_ERR_CAPACITY with the bit's text, the outputs complete. */
int olf_pose_optimization_rows(olf_ctx* ctx, const olf_pose_points_batch* in, int n_rows, int n_frames, const olf_pose_points_outputs* out);
/* tests: the LDS a workgroup may take for a row's edges (bytes; above it they live in context scratch; <= 0 restores the default) */
int olf_debug_pose_points_lds_limit(int bytes);

#ifdef __cplusplus
}
#endif
#endif
