/* orbline_types.h -- POD records and parameter blocks shared by the HIP library
 * (liborbline_hip.so), the C++ adaptor and the CPU oracle.
 *
 * Every record mirrors, field for field, a type that crosses the reference's
 * ORBextractor / Lineextractor / ORBmatcher / LineMatcher / Frame surfaces
 * (paths relative to /root/reference):
 *   olf_keypoint  == cv::KeyPoint (28 B) as filled by src/ORBextractor.cc:839-849,1097-1103
 *   olf_keyline   == cv::line_descriptor::KeyLine (68 B),
 *                    Thirdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:105-144
 *   descriptors   == rows of a continuous cv::Mat N x 32 CV_8U (src/ORBextractor.cc:1069,
 *                    Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:634)
 */
#ifndef ORBLINE_TYPES_H
#define ORBLINE_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLF_DESC_BYTES 32      /* 256-bit ORB and LBD descriptors                     */
#define OLF_MAX_LEVELS 16
#define OLF_GRID_COLS 64       /* include/Frame.h:51 FRAME_GRID_COLS                  */
#define OLF_GRID_ROWS 48       /* include/Frame.h:52 FRAME_GRID_ROWS                  */
#define OLF_GRID_CELLS 3072    /* OLF_GRID_COLS * OLF_GRID_ROWS                       */
#define OLF_GRID_MAX_KEYS 8192 /* key points per frame olf_frame_grid* sorts (their cells sit in LDS) */
/* Frame::mGrid as two arrays (std::vector<std::size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS], include/Frame.h:228; filled by
 * Frame::AssignFeaturesToGrid, src/Frame.cc:334-349) -- the one definition every producer and consumer of a grid cites:
 *   int32 cell_offsets[OLF_GRID_CELLS + 1], int32 cell_index[cell_offsets[OLF_GRID_CELLS]]
 *   - cell (ix, iy) = mGrid[ix][iy] is entry ix * OLF_GRID_ROWS + iy: its features are cell_index[cell_offsets[e] .. cell_offsets[e + 1]), so the
 *     cells iy0 .. iy1 of one column are one contiguous range;
 *   - inside a cell the feature indices ascend (the reference's push_back order);
 *   - a feature whose PosInGrid (src/Frame.cc:572-582) is false is in no cell: cell_offsets[OLF_GRID_CELLS] <= N;
 *   - entries of cell_index past cell_offsets[OLF_GRID_CELLS] are unspecified. */

typedef struct olf_keypoint {
    float x, y;        /* pt, level-0 pixel coordinates                                 */
    float size;        /* (int)(31*scale[octave])                                       */
    float angle;       /* degrees [0,360)                                               */
    float response;    /* FAST score                                                    */
    int32_t octave;
    int32_t class_id;  /* -1, as cv::KeyPoint's default                                 */
} olf_keypoint;

typedef struct olf_keyline {
    float angle;
    int32_t class_id;
    int32_t octave;
    float pt_x, pt_y;
    float response;
    float size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength;
    int32_t numOfPixels;
} olf_keyline;

/* one call of Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel), src/Frame.cc:517-570 (include/Frame.h:117: the levels default to -1, -1) */
typedef struct olf_area_query {
    float x, y, r;
    int32_t min_level, max_level;
} olf_area_query;

/* One snapshot of the map as Tracking::UpdateLocalMap walks it (src/Tracking.cc:2028-2205; olf_update_local_map*, include/orbline.h).  Key frames, map
 * points and map lines are numbered by the caller; every index array is int32, every flag array uint8.  A CSR pair is offsets [n + 1], non-decreasing from
 * 0, and index [offsets[n]].  Convention C.16: ascending key-frame index stands for ascending KeyFrame* address. */
typedef struct olf_map_graph {
    int32_t n_kf, n_mp, n_ml;
    const int32_t* mp_obs_offsets;    /* [n_mp + 1]  MapPoint::GetObservations() of every map point as key-frame indices;          */
    const int32_t* mp_obs_kf;         /*             the order inside a point is irrelevant                                        */
    const uint8_t* mp_bad;            /* [n_mp]      MapPoint::isBad()                                                             */
    const uint8_t* ml_bad;            /* [n_ml]      MapLine::isBad()                                                              */
    const uint8_t* kf_bad;            /* [n_kf]      KeyFrame::isBad()                                                             */
    const int32_t* kf_mp_offsets;     /* [n_kf + 1]  KeyFrame::GetMapPointMatches() in slot order as map-point indices,            */
    const int32_t* kf_mp_index;       /*             negative = NULL                                                               */
    const int32_t* kf_ml_offsets;     /* [n_kf + 1]  KeyFrame::GetMapLineMatches() in the same form; n_ml == 0 with ml_bad and     */
    const int32_t* kf_ml_index;       /*             both of these NULL: a map without lines                                       */
    const int32_t* kf_covis_offsets;  /* [n_kf + 1]  mvpOrderedConnectedKeyFrames in its order (GetVectorCovisibleKeyFrames());    */
    const int32_t* kf_covis_index;    /*             the first 10 of a row are read (GetBestCovisibilityKeyFrames(10))             */
    const int32_t* kf_child_offsets;  /* [n_kf + 1]  KeyFrame::GetChilds(), every row strictly ascending (C.16)                    */
    const int32_t* kf_child_index;
    const int32_t* kf_parent;         /* [n_kf]      KeyFrame::GetParent(), -1 = none                                              */
} olf_map_graph;

/* What LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) reads beyond an olf_map_graph, passed beside it (olf_keyframe_culling*, include/orbline.h):
 * the observer's feature index of every observation, the observation counter of every point and the key point, depth and mode of every slot's key frame.
 * The observation row of a bad point is never read: MapPoint::SetBadFlag cleared it (src/MapPoint.cc:171), so what mp_obs_kf / mp_obs_slot hold there is
 * irrelevant. */
typedef struct olf_cull_view {
    const int32_t* mp_obs_slot;       /* parallel to mp_obs_kf: the size_t of mObservations, the observer's feature index          */
    const int32_t* mp_nobs;           /* [n_mp]      MapPoint::Observations(): +2 per stereo observation (src/MapPoint.cc:117-120),  */
                                      /*             so it is not the length of the observation row                                */
    const uint8_t* kf_slot_octave;    /* parallel to kf_mp_index: mvKeysUn[i].octave                                               */
    const float*   kf_slot_depth;     /* parallel to kf_mp_index: mvDepth[i]                                                       */
    const uint8_t* kf_slot_stereo;    /* parallel to kf_mp_index: mvuRight[i] >= 0; read by olf_keyframe_culling_replay only       */
    const float*   kf_th_depth;       /* [n_kf]      mThDepth                                                                      */
    const uint8_t* kf_mode;           /* [n_kf]      0 normal, 1 mbNotErase, 2 mnId == 0; read by olf_keyframe_culling_replay only */
} olf_cull_view;

/* ORBextractor ctor arguments, src/ORBextractor.cc:412-416; values from
 * Examples/PL/PL_KITTI00-02.yaml:42-55 are the defaults of olf_default_params(). */
typedef struct olf_orb_params {
    int32_t nfeatures;
    float   scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
    /* convention C.11: fixed-point Gaussian taps of the 7x7 sigma-2 blur.  0: every tap rounded on its own, [18,34,49,55,49,34,18],
     * sum 257 (OpenCV 3.4.0-3.4.5, the range the reference most plausibly linked); 1: error-diffused taps that sum to 256 exactly
     * (later releases' "bit-exact" kernel), [18,34,48,56,48,34,18] */
    int32_t conv_gauss_sum256;
} olf_orb_params;

/* Lineextractor 11-argument ctor (include/LineExtractor.h:44-45) -- the LSD options
 * forwarded at src/LineExtractor.cc:44-53. */
typedef struct olf_line_params {
    int32_t lsd_nfeatures;      /* 0 = keep all                                        */
    double  min_line_length;    /* relative to min(w,h); src/LineExtractor.cc:53       */
    int32_t lsd_refine;         /* 0 LSD_REFINE_NONE, 1 LSD_REFINE_STD, 2 LSD_REFINE_ADV */
    double  lsd_scale;
    double  lsd_sigma_scale;
    double  lsd_quant;
    double  lsd_ang_th;         /* degrees, (0, 180).  Up to 80 the growth agent decides alignment by dot / cross products under a proven margin */
    double  lsd_log_eps;
    double  lsd_density_th;
    int32_t lsd_n_bins;         /* 2 .. 2^24.  Up to 1024 bins and LSD working images below 2^22 pixels (round(lsd_scale w) x round(lsd_scale h)) take the
                                 * fast path; beyond either the 64-bit-key capacity path (csrc/lsd_wide.hip): same results, about 6 x the time */
    /* conventions where the un-vendored OpenCV decides the result and its version is not pinned by the reference:
     * C.11 conv_gauss_sum256: as in olf_orb_params, for LSD's sigma-0.6 blur and LBD's 5x5 sigma-1 blur.
     * C.10 conv_resize_exact: LSD's x1.2 upsampling, 0: cv::resize INTER_LINEAR (11-bit coefficients); 1: INTER_LINEAR_EXACT (8-bit
     *      coefficients, round-to-nearest at the end), which later 3.4.x releases of lsd.cpp call.
     * C.9  conv_seed_order: order of the seeds INSIDE a gradient bin.  1 (default): whatever std::sort(begin, end, norm descending) of
     *      libstdc++ leaves -- OpenCV >= 3.3 pushes every pixel as {point, bin} and calls the unstable std::sort; the reference's CMakeLists.txt
     *      asks for OpenCV 3.4 first.  The order is a property of libstdc++'s introsort run over the whole pixel sequence; csrc/lsd_seedsort.hip
     *      replays it bit-exactly (oracle: the real std::sort).  0: raster order (the linked-list pseudo-ordering of the original LSD and of
     *      OpenCV <= 3.2; a stable radix sort on the device). */
    int32_t conv_gauss_sum256;
    int32_t conv_resize_exact;
    int32_t conv_seed_order;
    /* C.6  conv_libm_float: the unqualified cos / sin / atan2 / sqrt calls on FLOAT arguments inside cv::LineSegmentDetector's region_grow
     *      (sumdx += cos(float(angle))), LSDDetectorC::detectImpl (kl.angle = atan2(dy, dx), LSDDetector_custom.cpp:298) and BinaryDescriptor::computeLBD
     *      (dL = cos / sin(direction), binary_descriptor_custom.cpp:1130-1131; 1 / sqrt(tempM), :1283-1341).  Which overload they resolve to depends on the
     *      headers of the build: 0 (default) = ::cos(double) etc. -- the C functions, result rounded to float by the assignment; 1 = the float overloads
     *      (cosf / sinf / atan2f / sqrtf and a float division), which libstdc++ >= 6 makes visible when <math.h> is included.  Both variants are restated
     *      in the oracle and on the device (glibc 2.35's cosf / sinf / atan2f bit for bit). */
    int32_t conv_libm_float;
} olf_line_params;

/* Camera / matching scalars read on the path:
 * src/Tracking.cc:54-79,156 ; src/Config.cpp:26-160 */
typedef struct olf_stereo_params {
    float  fx;                  /* Camera.fx                                           */
    float  bf;                  /* Camera.bf                                           */
    int32_t matching_s_ws;      /* Config::matchingSWs()                               */
    double line_sim_th;         /* Config::lineSimTh()                                 */
    double min_ratio_12_l;      /* Config::minRatio12L()                               */
    double min_disp;            /* Config::minDisp()                                   */
    double line_horiz_th;       /* Config::lineHorizTh()                               */
    double stereo_overlap_th;   /* Config::stereoOverlapTh()                           */
    double ls_min_disp_ratio;   /* Config::lsMinDispRatio()                            */
    int32_t best_lr_matches;    /* Config::bestLRMatches()                             */
    /* conv_eigen_recip: `le_l = le_l / std::sqrt(...)` on an Eigen::Vector3d (src/Frame.cc:939).  Eigen 3.2+ divides every coefficient (0, default);
     * the 3.0 / 3.1 line -- CMakeLists.txt:45 accepts 3.1.0 -- implements vector / scalar as a multiplication by the reciprocal computed once
     * (scalar_quotient1_impl for non-integer scalars): 1.  mvle_l differs in the last bit between the two. */
    int32_t conv_eigen_recip;
} olf_stereo_params;

/* The parameter block of olf_ctx_create.  It must be initialised by olf_default_params(), which stamps abi_version and struct_size;
 * olf_ctx_create refuses a block whose stamp differs from the library's (a caller built against an older header would otherwise hand over a
 * shorter struct, and the conv_* fields would be read from whatever follows it). */
#define OLF_ABI_VERSION 4u
typedef struct olf_params {
    uint32_t          abi_version;   /* OLF_ABI_VERSION of the header the caller was built with */
    uint32_t          struct_size;   /* sizeof(olf_params) as the caller sees it               */
    olf_orb_params    orb;
    olf_line_params   line;
    olf_stereo_params stereo;
} olf_params;

/* status codes returned by every entry point */
enum {
    OLF_OK = 0,
    OLF_ERR_INVALID = -1,     /* bad argument (null, size mismatch, non-8UC1 ...)      */
    OLF_ERR_CAPACITY = -2,    /* caller-supplied capacity too small                    */
    OLF_ERR_HIP = -3,         /* HIP runtime error, see olf_last_error()               */
    OLF_ERR_NODEVICE = -4     /* no gfx950 device visible                              */
};

#ifdef __cplusplus
}
#endif
#endif
