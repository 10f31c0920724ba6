"""Batched stereo front-end: the feature part of Frame::Frame (reference src/Frame.cc:136-221)
for many independent stereo pairs at once -- ExtractORB x2, ExtractLine x2, ComputeStereoMatches,
ComputeStereoMatches_Lines -- on one GPU.  Mirrors the members the reference's Tracking reads:
mvKeys / mvKeysRight / mDescriptors / mDescriptorsRight / mvuRight / mvDepth (+ the line members).
"""
import numpy as np
from . import _lib
import ctypes as C
from ._lib import KEYPOINT_DTYPE, KEYLINE_DTYPE, DESC_BYTES, FrameBuffers, check, lib, ptr


class StereoFrames:
    """Results of one batch; arrays are (n_pairs, capacity[, ...]) with per-pair counts."""

    def __init__(self):
        self.N = self.Nr = None
        self.mvKeys = self.mvKeysRight = self.mDescriptors = self.mDescriptorsRight = None
        self.mvuRight = self.mvDepth = None
        self.N_l = self.Nr_l = None
        self.mvKeys_Line = self.mvKeysRight_Line = self.mDescriptors_Line = self.mDescriptorsRight_Line = None
        self.line_matches_12 = self.mvDisparity_l = self.mvle_l = None

    def pair(self, i):
        n, nr = int(self.N[i]), int(self.Nr[i])
        d = self._pair_points(i, n, nr)
        if self.N_l is not None:
            nl, nrl = int(self.N_l[i]), int(self.Nr_l[i])
            d.update(mvKeys_Line=self.mvKeys_Line[i, :nl], mDescriptors_Line=self.mDescriptors_Line[i, :nl],
                     mvKeysRight_Line=self.mvKeysRight_Line[i, :nrl], mDescriptorsRight_Line=self.mDescriptorsRight_Line[i, :nrl],
                     line_matches_12=self.line_matches_12[i, :nl], mvDisparity_l=self.mvDisparity_l[i, :nl], mvle_l=self.mvle_l[i, :nl])
        return d

    def _pair_points(self, i, n, nr):
        return dict(mvKeys=self.mvKeys[i, :n], mDescriptors=self.mDescriptors[i, :n], mvKeysRight=self.mvKeysRight[i, :nr],
                    mDescriptorsRight=self.mDescriptorsRight[i, :nr], mvuRight=self.mvuRight[i, :n], mvDepth=self.mvDepth[i, :n])


class StereoFrontEnd:
    def __init__(self, params=None, width=1242, height=375, max_pairs=1):
        self.params = params or _lib.default_params()
        self.ctx = _lib.Context(self.params, width, height, 2 * max_pairs)
        self.width, self.height, self.max_pairs = width, height, max_pairs
        self._last_images = 0          # images of the last frames() call: what the context's device buffers hold (frame_grid)

    def stereo_points(self, images):
        """images: (2*n_pairs, H, W) uint8, image 2p = left, 2p+1 = right (host memory)."""
        images = np.ascontiguousarray(images)
        if images.dtype != np.uint8 or images.ndim != 3 or images.shape[0] % 2:
            raise TypeError("stereo_points: (2*n_pairs, H, W) uint8 expected")
        if images.shape[1:] != (self.height, self.width):
            # Frame::Frame throws when the sizes differ (src/Frame.cc:145-146)
            raise RuntimeError("[StereoFrame] Left and right images have different sizes")
        n_pairs = images.shape[0] // 2
        cap = self.ctx.orb_capacity
        kps = np.zeros((2 * n_pairs, cap), KEYPOINT_DTYPE)
        desc = np.zeros((2 * n_pairs, cap, DESC_BYTES), np.uint8)
        counts = np.zeros(2 * n_pairs, np.int32)
        ur = np.zeros((n_pairs, cap), np.float32)
        dp = np.zeros((n_pairs, cap), np.float32)
        check(lib().olf_stereo_points(self.ctx.handle, ptr(images), n_pairs, ptr(kps), ptr(desc), ptr(counts), ptr(ur), ptr(dp)),
              "olf_stereo_points")
        f = StereoFrames()
        f.N, f.Nr = counts[0::2].copy(), counts[1::2].copy()
        f.mvKeys, f.mvKeysRight = kps[0::2], kps[1::2]
        f.mDescriptors, f.mDescriptorsRight = desc[0::2], desc[1::2]
        f.mvuRight, f.mvDepth = ur, dp
        return f

    def stereo_points_on(self, images, kps, desc, counts, fill=None):
        """ComputeStereoMatches on the CALLER's key points: images (2*n_pairs, H, W) uint8 go through olf_orb_extract_dev (which leaves their pyramids in
        the context), its key point, descriptor and count buffers are overwritten with kps (2*n_pairs, capacity) / desc (2*n_pairs, capacity, 32) /
        counts (2*n_pairs,), and olf_stereo_points_dev runs on those.  fill: value the two outputs hold before the call.
        Returns (mvuRight, mvDepth), each (n_pairs, capacity)."""
        import torch
        from .matcher import _torch_stream
        images = np.ascontiguousarray(images)
        n = images.shape[0]
        cap = self.ctx.orb_capacity
        if images.dtype != np.uint8 or images.shape[1:] != (self.height, self.width) or n % 2 or n > 2 * self.max_pairs:
            raise TypeError("stereo_points_on: (2*n_pairs, H, W) uint8 images of the context's size expected")
        kps, desc = np.ascontiguousarray(kps, KEYPOINT_DTYPE), np.ascontiguousarray(desc, np.uint8)
        counts = np.ascontiguousarray(counts, np.int32)
        if kps.shape != (n, cap) or desc.shape != (n, cap, DESC_BYTES) or counts.shape != (n,) or counts.min(initial=0) < 0 or counts.max(initial=0) > cap:
            raise ValueError("stereo_points_on: kps (n, capacity), desc (n, capacity, 32), counts (n,) within the capacity expected")
        d_img = torch.from_numpy(images).cuda()
        d_kps = torch.zeros((n, cap, KEYPOINT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros((n, cap, DESC_BYTES), dtype=torch.uint8, device="cuda")
        d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        ur = torch.full((n // 2, cap), 0.0 if fill is None else float(fill), dtype=torch.float32, device="cuda")
        dp = ur.clone()
        with _torch_stream() as s:
            check(lib().olf_orb_extract_dev(self.ctx.handle, d_img.data_ptr(), n, d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), s),
                  "olf_orb_extract_dev")
        # (each `with` ends device-wide synchronised when torch is on its default stream: the copies land after the extractor's own results)
        d_kps.copy_(torch.from_numpy(kps.view(np.uint8).reshape(n, cap, -1)))
        d_desc.copy_(torch.from_numpy(desc))
        d_counts.copy_(torch.from_numpy(counts))
        with _torch_stream() as s:
            check(lib().olf_stereo_points_dev(self.ctx.handle, n // 2, d_kps.data_ptr(), d_desc.data_ptr(), d_counts.data_ptr(), ur.data_ptr(),
                                              dp.data_ptr(), s), "olf_stereo_points_dev")
        torch.cuda.synchronize()
        return ur.cpu().numpy(), dp.cpu().numpy()

    def stereo_lines(self, kls, ldesc, lcounts):
        """ComputeStereoMatches_Lines on already extracted key lines: kls (2*n_pairs, cap), ldesc, lcounts."""
        kls, ldesc = np.ascontiguousarray(kls), np.ascontiguousarray(ldesc)
        lcounts = np.ascontiguousarray(lcounts, np.int32)
        n_pairs = kls.shape[0] // 2
        cap = self.ctx.line_capacity
        assert kls.shape[1] == cap
        m12 = np.full((n_pairs, cap), -1, np.int32)
        disp = np.zeros((n_pairs, cap, 2), np.float32)
        le = np.zeros((n_pairs, cap, 3), np.float64)
        check(lib().olf_stereo_lines(self.ctx.handle, n_pairs, ptr(kls), ptr(ldesc), ptr(lcounts), ptr(m12), ptr(disp), ptr(le)), "olf_stereo_lines")
        return m12, disp, le

    def frames(self, images):
        """The whole feature part of Frame::Frame (src/Frame.cc:136-221) for (2*n_pairs, H, W) uint8 host images."""
        images = np.ascontiguousarray(images)
        if images.dtype != np.uint8 or images.ndim != 3 or images.shape[0] % 2:
            raise TypeError("frames: (2*n_pairs, H, W) uint8 expected")
        if images.shape[1:] != (self.height, self.width):
            raise RuntimeError("[StereoFrame] Left and right images have different sizes")
        n_pairs = images.shape[0] // 2
        cap, lcap = self.ctx.orb_capacity, self.ctx.line_capacity
        kps = np.zeros((2 * n_pairs, cap), KEYPOINT_DTYPE)
        desc = np.zeros((2 * n_pairs, cap, DESC_BYTES), np.uint8)
        counts = np.zeros(2 * n_pairs, np.int32)
        ur, dp = np.zeros((n_pairs, cap), np.float32), np.zeros((n_pairs, cap), np.float32)
        kls = np.zeros((2 * n_pairs, lcap), KEYLINE_DTYPE)
        ldesc = np.zeros((2 * n_pairs, lcap, DESC_BYTES), np.uint8)
        lcounts = np.zeros(2 * n_pairs, np.int32)
        lm = np.full((n_pairs, lcap), -1, np.int32)
        ldisp = np.zeros((n_pairs, lcap, 2), np.float32)
        lle = np.zeros((n_pairs, lcap, 3), np.float64)
        fb = FrameBuffers(*[a.ctypes.data for a in (kps, desc, counts, ur, dp, kls, ldesc, lcounts, lm, ldisp, lle)])
        check(lib().olf_stereo_frames(self.ctx.handle, ptr(images), n_pairs, C.byref(fb)), "olf_stereo_frames")
        f = StereoFrames()
        f.N, f.Nr = counts[0::2].copy(), counts[1::2].copy()
        f.mvKeys, f.mvKeysRight = kps[0::2], kps[1::2]
        f.mDescriptors, f.mDescriptorsRight = desc[0::2], desc[1::2]
        f.mvuRight, f.mvDepth = ur, dp
        f.N_l, f.Nr_l = lcounts[0::2].copy(), lcounts[1::2].copy()
        f.mvKeys_Line, f.mvKeysRight_Line = kls[0::2], kls[1::2]
        f.mDescriptors_Line, f.mDescriptorsRight_Line = ldesc[0::2], ldesc[1::2]
        f.line_matches_12, f.mvDisparity_l, f.mvle_l = lm, ldisp, lle
        self._last_images = 2 * n_pairs
        return f

    def frame_grid(self, bounds=None, img_stride=2, counts=None, fill=None, n_frames=None):
        """Frame::mGrid (AssignFeaturesToGrid, src/Frame.cc:334-349) of the frames of the last frames() call, built by olf_frame_grid_dev on the
        context's device buffers -- the key points are not uploaded again.  Frame j is image j * img_stride (2: the left images).  bounds =
        (mnMinX, mnMaxX, mnMinY, mnMaxY), default the image (0, width, 0, height).  counts: an int32 array over ALL images of the call that
        replaces the device counts (N per image; a frame can be shortened or emptied); fill: value the output arrays hold before the call;
        n_frames: build the first n_frames grids only (the rows of the others keep the fill value).
        Returns (cell_offsets [frames, 3073], cell_index [frames, capacity]) -- layout in include/orbline_types.h."""
        import torch
        n_images = self._last_images
        if not n_images:
            raise RuntimeError("frame_grid: no frames() call to take the key points from")
        all_frames = (n_images + img_stride - 1) // img_stride
        n_frames = all_frames if n_frames is None else int(n_frames)
        if not 0 <= n_frames <= all_frames:
            raise ValueError("frame_grid: n_frames exceeds the frames of the last frames() call")
        minX, maxX, minY, maxY = (0.0, float(self.width), 0.0, float(self.height)) if bounds is None else (float(v) for v in bounds)
        fb = FrameBuffers()
        check(lib().olf_ctx_device_buffers(self.ctx.handle, C.byref(fb)), "olf_ctx_device_buffers")
        d_counts, keep = fb.counts, None
        if counts is not None:
            counts = np.ascontiguousarray(counts, np.int32)
            if counts.shape != (n_images,):
                raise ValueError("frame_grid: counts has one entry per image of the last frames() call")
            keep = torch.from_numpy(counts).cuda()
            d_counts = keep.data_ptr()
        cap = self.ctx.orb_capacity
        offs = torch.full((all_frames, _lib.GRID_CELLS + 1), 0 if fill is None else int(fill), dtype=torch.int32, device="cuda")
        idx = torch.full((all_frames, cap), 0 if fill is None else int(fill), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()          # (the context's stream is not ordered with torch's)
        check(lib().olf_frame_grid_dev(self.ctx.handle, n_frames, int(img_stride), fb.kps, d_counts, minX, maxX, minY, maxY,
                                       C.c_void_p(offs.data_ptr()), C.c_void_p(idx.data_ptr()), None), "olf_frame_grid_dev")
        self.ctx.synchronize()
        return offs.cpu().numpy(), idx.cpu().numpy()

    def _last_frames(self, who):
        """(device buffers, number of left frames) of the last frames() call"""
        if not self._last_images:
            raise RuntimeError(f"{who}: no frames() call to take the features from")
        fb = FrameBuffers()
        check(lib().olf_ctx_device_buffers(self.ctx.handle, C.byref(fb)), "olf_ctx_device_buffers")
        return fb, self._last_images // 2

    def stereo_points_mask(self):
        """mvDepth > 0 of the last frames() call as a device byte mask [n_pairs, capacity] (olf_stereo_points_mask_dev): the map points a frame owns
        right after stereo matching, i.e. mp_valid of search_by_projection_batch."""
        import torch
        fb, n = self._last_frames("stereo_points_mask")
        from .matcher import _torch_stream
        mask = torch.zeros((n, self.ctx.orb_capacity), dtype=torch.uint8, device="cuda")
        with _torch_stream() as s:
            check(lib().olf_stereo_points_mask_dev(self.ctx.handle, fb.depth, n * self.ctx.orb_capacity, C.c_void_p(mask.data_ptr()), s),
                  "olf_stereo_points_mask_dev")
        return mask

    def unproject_stereo(self, camera, Twc):
        """Frame::UnprojectStereo (src/Frame.cc:1073-1087) for every left-image feature of the last frames() call, on the context's device buffers
        (olf_unproject_stereo_dev).  camera = (fx, fy, cx, cy); Twc [n_pairs, 4, 4] float32, camera to world (rows of mRwc | mOw), numpy or device
        tensor.  Returns world [n_pairs, capacity, 3] as a device tensor."""
        import torch
        from . import matcher
        fb, n = self._last_frames("unproject_stereo")
        Twc = torch.as_tensor(np.ascontiguousarray(Twc, np.float32) if isinstance(Twc, np.ndarray) else Twc).cuda().contiguous()
        if tuple(Twc.shape) != (n, 4, 4):
            raise ValueError("unproject_stereo: Twc has one 4 x 4 matrix per stereo pair of the last frames() call")
        return matcher.unproject_stereo(n, fb.kps, fb.counts, fb.depth, camera, Twc, img_stride=2, context=self.ctx)

    def search_by_projection_batch(self, Tcw, mp_world, camera, th, bMono=False, checkOri=True, bounds=None, mp_valid=None, mp_obs=None,
                                   outlier=None, mp_desc=None, d_th=None, match12=True, out=None):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono[, match12]) between consecutive left frames of the last frames() call,
        on the context's device buffers (olf_search_by_projection_batch_dev; the grids come from olf_frame_grid_dev in the same call, nothing is
        downloaded).  Tcw [n_pairs, 4, 4] float32 (numpy or device tensor); mp_world [n_pairs, capacity, 3] device tensor (unproject_stereo);
        camera = (fx, fy, cx, cy, mbf); bounds default to the image; mp_valid e.g. stereo_points_mask().  The other arguments and the result
        (matches, match12, nmatches: device tensors over the n_pairs - 1 frame pairs) are those of matcher.search_by_projection_batch."""
        import torch
        from . import matcher
        fb, n = self._last_frames("search_by_projection_batch")
        cap = self.ctx.orb_capacity
        minX, maxX, minY, maxY = (0.0, float(self.width), 0.0, float(self.height)) if bounds is None else (float(v) for v in bounds)
        Tcw = torch.as_tensor(np.ascontiguousarray(Tcw, np.float32) if isinstance(Tcw, np.ndarray) else Tcw).cuda().contiguous()
        if tuple(Tcw.shape) != (n, 4, 4):
            raise ValueError("search_by_projection_batch: Tcw has one 4 x 4 matrix per stereo pair of the last frames() call")
        offs = torch.zeros((n, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
        idx = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
        with matcher._torch_stream() as s:
            check(lib().olf_frame_grid_dev(self.ctx.handle, n, 2, fb.kps, fb.counts, minX, maxX, minY, maxY, C.c_void_p(offs.data_ptr()),
                                           C.c_void_p(idx.data_ptr()), s), "olf_frame_grid_dev")
        return matcher.search_by_projection_batch(n, fb.kps, fb.desc, fb.counts, fb.uright, offs, idx, Tcw, mp_world, camera, (minX, maxX, minY, maxY), th,
                                                  bMono=bMono, checkOri=checkOri, img_stride=2, mp_valid=mp_valid, mp_obs=mp_obs, outlier=outlier,
                                                  mp_desc=mp_desc, d_th=d_th, match12=match12, out=out, context=self.ctx)

    def search_for_triangulation_batch(self, voc, Tcw, pairs, F12, camera, Cw=None, mp_valid=None, bOnlyStereo=False, checkOri=True, levelsup=4, out=None):
        """ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:659-825) for a list of pairs of the left frames of the last frames() call, on the
        context's device buffers (olf_search_for_triangulation_batch_dev; nothing is downloaded).  voc: an ORBVocabulary; Tcw [n_pairs, 4, 4] float32
        (numpy or device tensor), one per stereo pair; pairs int32 [n, 2] = (kf1, kf2) frame indices and F12 float32 [n, 3, 3] (numpy or device
        tensors); camera = (fx, fy, cx, cy); mp_valid e.g. stereo_points_mask().  The other arguments and the result (matches12, nmatches: device
        tensors over the listed pairs) are those of matcher.search_for_triangulation_batch."""
        import torch
        from . import matcher
        fb, n = self._last_frames("search_for_triangulation_batch")
        dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dt) if isinstance(a, np.ndarray) else a).cuda().contiguous()
        Tcw = dev(Tcw, np.float32)
        if tuple(Tcw.shape) != (n, 4, 4):
            raise ValueError("search_for_triangulation_batch: Tcw has one 4 x 4 matrix per stereo pair of the last frames() call")
        return matcher.search_for_triangulation_batch(voc, n, fb.kps, fb.desc, fb.counts, fb.uright, Tcw, dev(pairs, np.int32), dev(F12, np.float32), camera,
                                                      Cw=dev(Cw, np.float32), mp_valid=mp_valid, bOnlyStereo=bOnlyStereo, checkOri=checkOri,
                                                      levelsup=levelsup, img_stride=2, out=out, context=self.ctx)

    def search_by_bow_pairs(self, voc, pairs, mp_valid=None, mp_bad=None, form=0, nnratio=0.7, checkOri=True, levelsup=4, out=None):
        """ORBmatcher::SearchByBoW (src/ORBmatcher.cc:161-290, or :524-657 with form=matcher.BOW_KF_KF) for a list of pairs of the left frames of the
        last frames() call, on the context's device buffers (olf_search_by_bow_pairs_dev; nothing is downloaded).  voc: an ORBVocabulary; pairs int32
        [n, 2] = (first, second) frame indices (numpy or device tensor); mp_valid e.g. stereo_points_mask().  The other arguments and the result
        (matches, nmatches: device tensors over the listed pairs) are those of matcher.search_by_bow_pairs."""
        import torch
        from . import matcher
        fb, n = self._last_frames("search_by_bow_pairs")
        pairs = torch.as_tensor(np.ascontiguousarray(pairs, np.int32) if isinstance(pairs, np.ndarray) else pairs).cuda().contiguous()
        return matcher.search_by_bow_pairs(voc, n, fb.kps, fb.desc, fb.counts, pairs, mp_valid=mp_valid, mp_bad=mp_bad, form=form, nnratio=nnratio,
                                           checkOri=checkOri, levelsup=levelsup, img_stride=2, out=out, context=self.ctx)

    def search_local_map_batch(self, Tcw, local_map, camera, th=1.0, nnratio=0.8, viewingCosLimit=0.5, bounds=None, frame_mp=None, d_th=None, out=None):
        """The point half of Tracking::SearchLocalPointsAndLines (src/Tracking.cc:1877-1942) for the left frames of the last frames() call, on the
        context's device buffers: olf_frame_grid_dev, then olf_search_local_map_batch_dev -- nothing is downloaded.  Tcw [n_pairs, 4, 4] float32
        (numpy or device tensor); local_map: a matcher.LocalMapDev; camera = (fx, fy, cx, cy, mbf); bounds default to the image.  The other
        arguments and the result (matches [n_pairs, capacity] as map indices, nmatches [n_pairs]: device tensors) are those of
        matcher.search_local_map_batch."""
        import torch
        from . import matcher
        fb, n = self._last_frames("search_local_map_batch")
        cap = self.ctx.orb_capacity
        minX, maxX, minY, maxY = (0.0, float(self.width), 0.0, float(self.height)) if bounds is None else (float(v) for v in bounds)
        Tcw = torch.as_tensor(np.ascontiguousarray(Tcw, np.float32) if isinstance(Tcw, np.ndarray) else Tcw).cuda().contiguous()
        if tuple(Tcw.shape) != (n, 4, 4):
            raise ValueError("search_local_map_batch: Tcw has one 4 x 4 matrix per stereo pair of the last frames() call")
        offs = torch.zeros((n, _lib.GRID_CELLS + 1), dtype=torch.int32, device="cuda")
        idx = torch.zeros((n, cap), dtype=torch.int32, device="cuda")
        with matcher._torch_stream() as s:
            check(lib().olf_frame_grid_dev(self.ctx.handle, n, 2, fb.kps, fb.counts, minX, maxX, minY, maxY, C.c_void_p(offs.data_ptr()),
                                           C.c_void_p(idx.data_ptr()), s), "olf_frame_grid_dev")
        return matcher.search_local_map_batch(n, fb.kps, fb.desc, fb.counts, fb.uright, offs, idx, Tcw, local_map, camera, (minX, maxX, minY, maxY), th=th,
                                              nnratio=nnratio, viewingCosLimit=viewingCosLimit, frame_mp=frame_mp, d_th=d_th, img_stride=2, out=out,
                                              context=self.ctx)


def assign_features_to_grid(keys, bounds, context=None):
    """Frame::AssignFeaturesToGrid (src/Frame.cc:334-349) for one frame's key points (KEYPOINT_DTYPE, mvKeysUn) on the device: olf_frame_grid.
    bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY).  Returns (cell_offsets [3073], cell_index [cell_offsets[-1]]): cell (ix, iy) = mGrid[ix][iy] holds
    cell_index[cell_offsets[ix * 48 + iy] : cell_offsets[ix * 48 + iy + 1]]."""
    from .matcher import _ctx
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    offs, idx = np.zeros(_lib.GRID_CELLS + 1, np.int32), np.zeros(max(len(keys), 1), np.int32)
    check(lib().olf_frame_grid(_ctx(context).handle, ptr(keys), len(keys), *(float(v) for v in bounds), ptr(offs), ptr(idx)), "olf_frame_grid")
    return offs, idx[:offs[-1]].copy()


def features_in_area(keys, grid, bounds, queries, capacity=None, context=None):
    """Frame::GetFeaturesInArea (src/Frame.cc:517-570) for many queries on the device: olf_features_in_area.  grid = (cell_offsets, cell_index) of
    `keys` under `bounds`; queries: AREA_QUERY_DTYPE records (x, y, r, min_level, max_level; the reference's default levels are -1, -1).
    Returns the CSR (cand_offsets [n_queries + 1], cand_idx) olf_match_candidates consumes: query q's vIndices, in the reference's order, are
    cand_idx[cand_offsets[q] : cand_offsets[q + 1]].  capacity: size of the index buffer (default: sized by a first call with none)."""
    from .matcher import _ctx
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    offs, idx = np.ascontiguousarray(grid[0], np.int32), np.ascontiguousarray(grid[1], np.int32)
    if offs.shape != (_lib.GRID_CELLS + 1,):
        raise ValueError("features_in_area: cell_offsets has OLF_GRID_CELLS + 1 entries")
    queries = np.ascontiguousarray(np.asarray(queries, _lib.AREA_QUERY_DTYPE).reshape(-1))
    h, b = _ctx(context).handle, [float(v) for v in bounds]

    def run(cap):
        co, ci = np.zeros(len(queries) + 1, np.int32), np.zeros(max(cap, 1), np.int32)
        rc = lib().olf_features_in_area(h, ptr(keys), len(keys), ptr(offs), ptr(idx), *b, len(queries), ptr(queries), ptr(co), ptr(ci), cap)
        return rc, co, ci
    rc, co, ci = run(0 if capacity is None else int(capacity))
    if capacity is None and rc == _lib.OLF_ERR_CAPACITY:           # the offsets are complete: they size the second call
        rc, co, ci = run(int(co[-1]))
    check(rc, "olf_features_in_area")
    return co, ci[:co[-1]].copy()
