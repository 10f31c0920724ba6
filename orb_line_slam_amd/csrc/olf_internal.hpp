// olf_internal.hpp -- what every translation unit of the library shares: the geometry and device buffers of the ORB side, the launchers, the ctx_*
// accessors and the scratch slots.  The context itself (struct olf_ctx) is ctx.hpp, seen by api.cpp, api_host.cpp and api_debug.cpp only.
//
// One olf_ctx serves a fixed image size (w x h), a fixed parameter block and up to max_images
// images per call (a stereo pair = 2 images: index 2*pair + side).  All buffers are allocated once
// at creation and sized for the worst case, so the hot path never allocates; with 288 GB of HBM3E
// a context for hundreds of KITTI pairs is a few GB.
//
// HBM layout (per image, all level images packed with a 64-byte aligned pitch):
//   pyr   : u8  levels 0..L-1   (level 0 is an aligned copy of the input)      mvImagePyramid
//   blur  : u8  levels 0..L-1   GaussianBlur(7x7, sigma 2) of pyr               workingMat
//   cells : u32 per FAST cell a slot of cell_cap packed candidates (x:12 | y:12 | score:8, cell-local
//           coordinates are converted to level coordinates relative to minBorder) + one count
//   cand  : u32 per level, candidates gathered in reference order (vToDistributeKeys)
//   lvl_kp: u32 per level, octree survivors in lNodes order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/orbline_types.h"
#include "device_math.hpp"      // OLF_HD

#define OLF_HIP_CHECK(expr)                                                                 \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            olf::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));              \
            return OLF_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

#define OLF_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != OLF_OK) return _rc; \
    } while (0)

struct olf_ctx;

namespace olf {

void set_error(const std::string& s);

// The context's four grow-on-demand scratch slabs.  An entry carves its slot (staging.hpp) and the slab is in use until the last kernel or copy the
// entry enqueued has run, so two entries may share a slot only when their work is ordered: on one stream, or with a synchronise between them.
//   SCRATCH_KNN    olf_match_bf_dev: the k-NN tables of launch_match_bf.
//   SCRATCH_STAGE  the descriptor-sized host-pointer entries (api_host.cpp: olf_match_bf, olf_knn2, olf_match_candidates, olf_frame_grid,
//                  olf_features_in_area, olf_hamming_matrix, olf_distinctive_descriptors; localmap_api.cpp: olf_update_local_map; connections_api.cpp: olf_update_connections; culling_api.cpp: olf_keyframe_culling,
//                  olf_tracked_map_points, olf_map_point_culling; pose_api.cpp: olf_pose_optimization_with_line_frame, olf_discard_outliers_frame; posepoints_api.cpp: olf_pose_optimization_rows; newpoints_api.cpp: olf_compute_f12_pairs,
//                  olf_create_new_map_points_pairs, olf_update_normal_and_depth_points) and the olf_debug_*_sweep counters.  Every one of them ends in
//                  a synchronise on the context's stream.
//   SCRATCH_BATCH  the batched matchers (olf_search_by_bow_batch_dev, olf_search_by_projection_batch_dev, olf_is_in_frustum_batch_dev,
//                  olf_search_local_map_batch_dev, olf_search_for_triangulation_batch_dev, olf_fuse_search_batch_dev, olf_search_by_sim3_pairs_dev,
//                  olf_search_by_projection_kf_pairs_dev, olf_search_by_projection_sim3_batch_dev, olf_update_local_map_batch_dev, olf_update_connections_batch_dev,
//                  olf_pose_optimization_with_line_batch_dev above the LDS a frame's state fits in, olf_pose_optimization_batch_dev likewise, olf_sim3_solver_pairs_dev (its table of iteration caps, and
//                  the correspondences above the LDS they fit in), olf_pnp_solver_pairs_dev (its table of parameters, and the correspondences above the LDS they fit in), olf_initializer_pairs_dev (the correspondences above the LDS they fit in), and the line entries of line_batch.hip) and the image-sized host-pointer entries (olf_cvt_gray, olf_remap_linear,
//                  olf_init_undistort_rectify_map, olf_bow_transform).  The matchers do not synchronise: the caller keeps them on one stream.
//   SCRATCH_PACK   olf_frames_pack_dev: the record's row offsets.
// Live at the same time: STAGE over KNN inside olf_match_bf (it stages, then calls olf_match_bf_dev); KNN, BATCH and PACK in a pipeline step that
// enqueues SearchByBoW, the line match and the packer behind one frame call without a synchronise (bench.py).  A slot number is a
// context's memory: moving an entry to another slot changes what a context allocates.
enum ScratchSlot { SCRATCH_KNN, SCRATCH_STAGE, SCRATCH_BATCH, SCRATCH_PACK, SCRATCH_SLOTS };

// what the entry points outside api*.cpp need of a context (api.cpp; the context itself is ctx.hpp, which no .hip file includes)
hipStream_t ctx_stream(olf_ctx* c, void* stream = nullptr);      // the caller's stream, or the context's own when the caller passes none
int ctx_scratch(olf_ctx* c, ScratchSlot slot, size_t bytes, void** out);
int* ctx_status(olf_ctx* c);
int ctx_check_device(const olf_ctx* c, const char* who);
int ctx_check_status(olf_ctx* c);                      // reads the device's capacity flags: OLF_OK, or OLF_ERR_CAPACITY with the flags cleared and named
// line outputs of a frame call whose line path is still running (olf_ctx_set_deferred_join): when one of the pointers lies in them, stream s waits for it first
int ctx_join_line_outputs(olf_ctx* c, hipStream_t s, const void* p0, const void* p1, const void* p2, const void* p3);
int ctx_level_scales(const olf_ctx* c, float* sf);     // mvScaleFactors into sf[0 .. OLF_MAX_LEVELS), 1.0 above the context's levels; returns the level count
int ctx_level_inv_sigma2(const olf_ctx* c, float* inv_sigma2);      // mvInvLevelSigma2 = 1.0f / (sf * sf), both in float, into [0 .. OLF_MAX_LEVELS); the level count
int ctx_level_thresholds(olf_ctx* c, float* thr);     // the table of olf_predict_scale_thresholds for the context's levels, built once

// The bits of the context's status word (ctx_status) that the batched matchers set, as every entry means them; include/orbline.h says per entry what was
// left out.  What a bit means is its row of kStatusText, which is also what check_status (api.cpp) tells the caller about a set bit.
enum StatusBit : int { STATUS_OCTAVE = 256, STATUS_POINT_INDEX = 512, STATUS_LINE_INDEX = 1024, STATUS_PAIR = 2048, STATUS_KF_INDEX = 4096, STATUS_LOCALMAP_LIST = 8192,
                       STATUS_CONNECTIONS_LIST = 16384 };
struct StatusText { int bit; const char* text; };
constexpr StatusText kStatusText[] = {
    {1, "ORB corner buffer"},
    {2, "ORB candidate buffer"},
    {4, "ORB key point buffer"},
    {8, "LSD regions, segments or pixel-list pool"},
    {16, "LSD growth watchdog"},
    {32, "frame record buffer"},
    {64, "LSD seed sort, final-range list of the grid-wide top levels"},
    {128, "candidate list of olf_features_in_area_dev"},
    {STATUS_OCTAVE, "a batched matcher left out a pair or a candidate that holds an octave outside the context's levels"},
    {STATUS_POINT_INDEX, "a batched point entry left out a list index or a per-frame map-point index outside the map"},
    {STATUS_LINE_INDEX, "a batched line entry left out a list index or a per-frame map-line index outside the map"},
    {STATUS_PAIR, "a pair entry skipped a pair whose frame indices are outside the batch or equal"},
    {STATUS_KF_INDEX, "a map-graph entry left out a key-frame index outside the graph"},
    {STATUS_LOCALMAP_LIST, "local key-frame, map-point or map-line list of olf_update_local_map_batch_dev"},
    {STATUS_CONNECTIONS_LIST, "connected or ordered key-frame list of olf_update_connections_batch_dev, or a row of olf_best_covisibles_batch_dev"},
};
// raise a status bit: the context's word on the device (atomic), the caller's on the host
OLF_HD void status_raise(int* status, int bit)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(status, bit);
#else
    *status |= bit;
#endif
}

// Row k of a CSR of n rows, inside [0, offs[n]] whatever the offsets hold: malformed offsets read nothing out of bounds.  csr_clamp is the form for a
// caller that holds total = max(offs[n], 0) already.
OLF_HD void csr_clamp(const int* __restrict__ offs, int k, int total, int& b, int& e)
{
    const int ob = offs[k], oe = offs[k + 1], lo = ob > 0 ? ob : 0, first = lo < total ? lo : total, hi = oe > first ? oe : first;
    b = first;                       // min(max(ob, 0), total)
    e = hi < total ? hi : total;     // min(max(oe, b), total)
}
OLF_HD void csr_row(const int* __restrict__ offs, int n, int k, int& b, int& e) { const int last = offs[n]; csr_clamp(offs, k, last > 0 ? last : 0, b, e); }

// What a slot holds, as an index into a map of n_items: v itself, or -1 for NULL (negative), an index outside the map (which raises `bit` of *status)
// or a bad item.
OLF_HD int live_item(int v, int n_items, const uint8_t* __restrict__ bad, int* __restrict__ status, int bit)
{
    if (v >= n_items) { status_raise(status, bit); return -1; }
    return v < 0 || bad[v] ? -1 : v;
}

#ifdef __HIPCC__
// a pair (f1, f2) of a pair entry is searched when both are frames of the batch and differ; otherwise the entry skips it and sets STATUS_PAIR
__device__ __forceinline__ bool pair_in_batch(int f1, int f2, int n_frames) { return f1 >= 0 && f1 < n_frames && f2 >= 0 && f2 < n_frames && f1 != f2; }

// Wave-wide vote.  hip's __ballot() converts the predicate to an int first and compares that with 0 (a v_cndmask + v_cmp_ne pair per vote);
// the wave64 builtin takes the compare's lane mask as it is.
// sum over the 64 lanes of a wave, wave-uniform result: two quad permutes, the two row mirrors (DPP, no LDS), then the four rows' sums through scalar registers
__device__ __forceinline__ int wave_sum_i32(int v)
{
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);       // quad_perm [1, 0, 3, 2]
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);       // quad_perm [2, 3, 0, 1]
    v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xf, 0xf, true);      // row_half_mirror
    v += __builtin_amdgcn_mov_dpp(v, 0x140, 0xf, 0xf, true);      // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// minimum over the 64 lanes of a wave (signed), wave-uniform result: the same four DPP steps, then the four rows' minima through scalar registers
__device__ __forceinline__ int wave_min_i32(int v)
{
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ unsigned long long wave_vote(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// set bits of a lane mask below this lane (v_mbcnt pair; "__popcll(m & ((1ull << lane) - 1))" compiles to a 64-bit shift, two bit-field inserts and two counts)
__device__ __forceinline__ int wave_rank_below(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }
// this lane's bit of a (wave-uniform) lane mask as a predicate: the mask becomes the EXEC / select operand as it is, no per-lane shift and compare
__device__ __forceinline__ bool wave_bit(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
#endif

constexpr int kEdge = 19;          // EDGE_THRESHOLD   src/ORBextractor.cc:76
constexpr int kMinBorder = 16;     // EDGE_THRESHOLD-3 src/ORBextractor.cc:775
constexpr int kHalfPatch = 15;     // HALF_PATCH_SIZE  src/ORBextractor.cc:75
// A FAST candidate is one 32-bit word, 12 bits per coordinate relative to kMinBorder and 8 of score (k_fast_score, k_cells_sort, k_octree, k_describe): the
// largest coordinate of a level, side - 2 * kMinBorder - 4, must not exceed 4095.  Level 0 is the largest level; a larger image is refused at context creation.
constexpr int kMaxOrbSide = 4095 + 2 * kMinBorder + 4;
static_assert(kMaxOrbSide == 4131, "olf_ctx_create's message and include/orbline.h state this limit");

// Geometry of one pyramid level; identical for every image of the context.
struct LevelGeom {
    int w, h, pitch;        // level size; pitch is a multiple of 64
    int offset;             // byte offset of the level inside a per-image pyramid block
    int maxBorderX, maxBorderY;
    int nCols, nRows, wCell, hCell;   // FAST cell grid, src/ORBextractor.cc:783-789
    uint32_t wCellM, hCellM;          // ceil(2^20 / wCell), ceil(2^20 / hCell): v / cell == (v * M) >> 20 for 0 <= v < 2^14 (k_fast_score's cell of a corner without a division)
    int cellBase;           // index of this level's first cell in the per-image cell arrays
    int quota;              // mnFeaturesPerLevel[level]
    int nIni;               // DistributeOctTree root count
    float hX;               // DistributeOctTree root width
    float scale;            // mvScaleFactor[level]
    float inv_scale;        // mvInvScaleFactor[level]
    int patch_size;         // (int)(31*scale)
    int candBase;           // offset of this level in the per-image candidate array
    int candCap;            // capacity of this level's candidate array
    int kpBase, kpCap;      // per-level survivor array (kpCap = quota + 8)
    int resizeTabX, resizeTabY;  // offsets into the resize coefficient tables (level >= 1)
    int resizeTiled;             // 1: the LDS-tiled resize kernel's staging area covers every tile of this level
};

struct ResizeCoef { int16_t ofs; int16_t a0; int16_t a1; int16_t pad; };

struct OrbGeom {
    int nlevels;
    int W, H, in_pitch;
    int pyrBytes;           // per image
    int totalCells;         // per image
    int cellCap;            // candidates per cell slot
    int candTotal;          // per image
    int kpTotal;            // per image (sum of kpCap)
    int outCap;             // max key points per image returned (nfeatures + 4*nlevels)
    int iniTh, minTh;
    int maxNodes;           // power of two at or above the largest kpCap: above 2048 k_octree spills its lists to global memory (sizes octSpill)
    LevelGeom lv[OLF_MAX_LEVELS];
    int umax[16];
    int blurTaps[7];
};

// Host-side derivation of every table of ORBextractor::ORBextractor (src/ORBextractor.cc:412-472),
// of the level sizes (:1113-1114), of the cell grid (:775-789) and of the cv::resize
// coefficient tables.  Pure host code (host_tables.cpp), held by the context.
struct OrbHostTables {
    std::vector<float> sf, inv_sf, sigma2, inv_sigma2;
    std::vector<int> nPerLevel;
    OrbGeom geom;
    std::vector<ResizeCoef> rx, ry;    // concatenated over levels
    bool portrait = false;             // a level's octree would have round(width / height) == 0 root cells: the context describes and matches only
    int build(const olf_orb_params& p, int W, int H);
};

std::vector<int> gaussian_taps_q8(int n, double sigma, int sum256 = 0);
// fills coef[0..dn) for a 1-D cv::resize(INTER_LINEAR) axis: sn source samples, step `scale`
void resize_axis_coefs(int sn, int dn, double scale, bool clamp_like_x, ResizeCoef* coef);

// ----------------------------------------------------------------------------------------------
struct OrbDeviceBufs {
    uint8_t* pyr = nullptr;       // [max_images][pyrBytes]
    uint8_t* blur = nullptr;
    uint32_t* cells = nullptr;    // [max_images][totalCells][cellCap]
    int* cellCount = nullptr;     // [max_images][totalCells]
    uint32_t* cand = nullptr;     // [max_images][candTotal]
    uint16_t* candNode = nullptr; // [max_images][candTotal]
    int* candCount = nullptr;     // [max_images][nlevels]
    uint32_t* lvlKp = nullptr;    // [max_images][kpTotal]
    int* lvlCount = nullptr;      // [max_images][nlevels]
    float* lvlAngle = nullptr;    // [max_images][kpTotal]
    ResizeCoef* rx = nullptr;
    ResizeCoef* ry = nullptr;
    OrbGeom* geom = nullptr;      // device copy
    int* status = nullptr;        // device error flags (capacity overflow etc.)
    unsigned char* octSpill = nullptr;   // [max_images][nlevels][octree_spill_bytes] only when maxNodes > 2048 (orb_octree.hip)
};

// kernel launchers (orb_*.hip)
int launch_orb_pyramid(const OrbGeom& g, const OrbDeviceBufs& b, const uint8_t* d_in, int n_images, hipStream_t s);
int launch_orb_fast(const OrbGeom& g, const OrbDeviceBufs& b, int n_images, hipStream_t s);
int launch_orb_octree(const OrbGeom& g, const OrbDeviceBufs& b, int n_images, hipStream_t s);
// k_octree's working set of one level (orb_octree.hip), the same on both sides of the launch.  The arrays hold exactly the level's capacity, so the kernel
// rests on this bound: the first sweep divides at most nIni roots (4 * nIni nodes); a later full sweep runs only while size + 3 * expandable <= quota and so
// ends with at most quota nodes; a careful round stops at the first division that reaches the quota, which adds at most 3 (quota + 2 nodes).  All are below
// kpCap = max(quota + 8, 4 * nIni + 4).  A careful round sorts the expandable nodes of a list that is still shorter than the quota.
__host__ __device__ inline int octree_node_cap(const LevelGeom& L) { return (L.kpCap + 7) & ~7; }
__host__ __device__ inline int octree_sort_cap(const LevelGeom& L)
{
    int s = 64;
    while (s < L.quota) s <<= 1;
    return s;
}
__host__ __device__ inline size_t octree_lds_bytes(int nodeCap, int sortCap) { return (size_t)nodeCap * 62 + (size_t)sortCap * 4; }
size_t octree_spill_bytes(const OrbGeom& g);      // per (image, level) slice of octSpill
// The launches of k_octree for a geometry (host_tables.cpp), at most three, the largest request first.  A launch carries one dynamic LDS size, so the levels are
// grouped by what their lists need: above 36 KB, 18 to 36 KB, at most 18 KB.  The LSD growth agents that run beside this kernel in the fused frame call hold
// 5120 B of LDS each, 24 of them a CU, which leaves 40 KB of the 160 KB: a level of the middle group fits once beside them, one of the small group twice, and
// neither waits with a larger level's request.  With maxNodes > 2048 it is one launch of every level with no LDS (the lists live in octSpill).
struct OctLevels { int n; int id[OLF_MAX_LEVELS]; };
struct OctLaunch { OctLevels lv; size_t lds; };
int octree_launches(const OrbGeom& g, OctLaunch out[3]);
int launch_orb_blur(const OrbGeom& g, const OrbDeviceBufs& b, int n_images, hipStream_t s);
int launch_orb_describe(const OrbGeom& g, const OrbDeviceBufs& b, int n_images, olf_keypoint* d_kps, uint8_t* d_desc,
                        int* d_counts, int out_cap, hipStream_t s);

// filters.hip
struct Taps7 { int t[7]; };
int launch_sep7(const uint8_t* src, size_t srcImgStride, int srcPitch, uint8_t* dst, size_t dstImgStride, int dstPitch, int W, int H,
                const int* taps7, int n_images, hipStream_t s);
int launch_sep_wide(const uint8_t* src, size_t srcImgStride, int srcPitch, uint8_t* dst, size_t dstImgStride, int dstPitch, int W, int H,
                    const int* taps, int r, int n_images, hipStream_t s);

bool resize_tiled_fits(const ResizeCoef* rx, const ResizeCoef* ry, int sw, int sh, int dw, int dh);
bool resize_strip_fits(const ResizeCoef* rx, int sw, int dw, int ncols = 4);      // the register-only kernel (bit 1 of resizeTiled; ncols = 5: the fused LSD kernel, bit 2)
int launch_resize_tiled(const uint8_t* src, size_t srcImgStride, int srcPitch, int sw, int sh, uint8_t* dst, size_t dstImgStride, int dstPitch,
                        int dw, int dh, const ResizeCoef* d_rx, const ResizeCoef* d_ry, int n_images, hipStream_t s, bool strip = false);

// precond.hip
int launch_cvt_gray(const uint8_t* src, uint8_t* dst, int w, int h, int code, int n_images, hipStream_t s);
int launch_init_rectify_map(const double* ir9, const double* k8, double fx, double fy, double u0, double v0, int w, int h, float* d_map1, float* d_map2,
                            hipStream_t s);
int launch_remap_linear(const uint8_t* src, int sw, int sh, const float* mapx, const float* mapy, int dw, int dh, uint8_t* dst, int n_images,
                        hipStream_t s);

// match.hip
int launch_stereo_points(const OrbGeom& g, const OrbDeviceBufs& b, int n_pairs, const olf_keypoint* d_kps, const uint8_t* d_desc,
                         const int* d_counts, int cap, float mbf, float fx, float* d_uRight, float* d_depth, int* d_sad, int* d_bestKey,
                         unsigned* d_perm, hipStream_t s);
int launch_match_bf(const uint8_t* dA, const int* nA, int strideA, int aStep, const uint8_t* dB, const int* nB, int strideB, int bStep,
                    int n_sets, float nnr, int best_lr, int* ws, int* m12, hipStream_t s);
int launch_knn2(const uint8_t* dA, const int* nA, int strideA, const uint8_t* dB, const int* nB, int strideB, int n_sets, int* idx0,
                int* dist0, int* dist1, hipStream_t s);
// kNN(2) of queries fetched through an index (k_knn2_indexed): set s has nQ[s] queries, query r = row qidx[rank_entry[qbase[s] + r]] of q, against the nT[s * tStep]
// (<= tCap <= 4096) rows at t + s * strideT * 32; results at place qbase[s] + r.  tile_prefix [n_sets + 1]: running sum of ceil(nQ[s] / 256), <= max_tiles
int launch_knn2_indexed(const uint8_t* q, const int* rank_entry, const int* qidx, const int* qbase, const int* nQ, const int* tile_prefix, int n_sets,
                        int max_tiles, const uint8_t* t, const int* nT, int strideT, int tStep, int tCap, int* idx0, int* dist0, int* dist1, hipStream_t s);
int launch_match_candidates(const uint8_t* q, int nQ, const uint8_t* t, int nT, const int* offs, const int* cand, uint16_t* out, hipStream_t s);
int launch_distinctive(const uint8_t* desc, const int* offs, int n_points, int* best, hipStream_t s);
int launch_hamming_matrix(const uint8_t* a, int nA, const uint8_t* b, int nB, uint16_t* out, hipStream_t s);


// grid.hip
// mfGridElementWidthInv / mfGridElementHeightInv, src/Frame.cc:186-187: static_cast<float>(FRAME_GRID_COLS) / (mnMaxX - mnMinX), in float; false for empty bounds
inline bool grid_scales(float minX, float maxX, float minY, float maxY, float* wInv, float* hInv)
{
    if (!(maxX > minX) || !(maxY > minY)) return false;
    *wInv = static_cast<float>(OLF_GRID_COLS) / (maxX - minX);
    *hInv = static_cast<float>(OLF_GRID_ROWS) / (maxY - minY);
    return true;
}
int launch_assign_grid(const olf_keypoint* d_kps, size_t frame_stride, const int* d_counts, int count_stride, int n_fixed, int n_limit, float minX,
                       float minY, float wInv, float hInv, int n_frames, int* d_cell_offsets, int* d_cell_index, size_t index_stride, hipStream_t s);
int launch_features_in_area(const olf_keypoint* d_keys, const int* d_cell_offsets, const int* d_cell_index, float minX, float minY, float wInv, float hInv,
                            int n_queries, const olf_area_query* d_queries, int* d_cand_offsets, int* d_cand_idx, int cand_capacity, int* d_status,
                            hipStream_t s);
// a caller-supplied Frame::mGrid (layout: orbline_types.h) for n features, checked in O(OLF_GRID_CELLS + n): offsets monotone from 0, last <= n, indices in [0, n)
bool grid_is_valid(const int32_t* cell_offsets, const int32_t* cell_index, int n);

// kfdb.hip
// the tables of olf_kfdb_tables_dev for one vocabulary: n_queries CSR queries (d_qoff [n_queries + 1] on the device) against slots [d_beg[k], d_beg[k] + d_len[k])
int launch_kfdb_tables(const int* d_qoff, const int* d_qids, const double* d_qvals, int n_queries, const int* d_beg, const int* d_len, const int* d_ids,
                       const double* d_vals, int n_slots, int* d_common, int* d_first, double* d_score, hipStream_t s);
// d_score[i] = L1 score(a_i, b_i); a_len == nullptr: the first operands are a CSR (a_beg [n_a + 1]), else slots as the second operands are
int launch_bow_score_pairs(const int* d_pairs, int n_pairs, const int* a_beg, const int* a_len, int n_a, const int* a_ids, const double* a_vals,
                           const int* b_beg, const int* b_len, int n_b, const int* b_ids, const double* b_vals, double* d_score, hipStream_t s);

}  // namespace olf
