"""ORBmatcher mirror (U:src/ORBmatcher.cc) over liborbhip.so.

``DescriptorDistance`` is the SWAR popcount of the reference. ``match_bf`` applies the
acceptance rule shared by SearchByBoW / SearchForInitialization — best/second over the
train set, ``best <= TH_LOW`` and ``best < mfNNratio * second``, then the 30-bin rotation
histogram (ComputeThreeMaxima) when ``mbCheckOrientation`` — order-free over the whole
train set (the C3 brute-force matcher). ``SearchForInitialization`` is the reference function
itself, with its windowed, greedy (stealing) one-to-one semantics.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import (KP_DTYPE, FrameC, InitFrameC, LocalPointsC, NewPointsC, ProjLastC, StereoViewC, TriKeyFrameC,
                   TriParamsC, TriStereoKeyFrameC, torch_stream, Context, check, lib, ptr)


class ORBmatcher:
    TH_HIGH = 100
    TH_LOW = 50
    HISTO_LENGTH = 30

    def __init__(self, nnratio: float = 0.6, checkOri: bool = True, device: int = -1, ctx: Context | None = None):
        self.mfNNratio = float(nnratio)
        self.mbCheckOrientation = bool(checkOri)
        self.ctx = ctx or Context(device)
        self._lp_cache = None   # SearchLocalPoints: the C view of the last call's map-point arrays
        self.last_direction = None   # the stereo SearchByProjectionLastFrame's direction of motion

    @staticmethod
    def DescriptorDistance(a, b) -> int:
        a = np.ascontiguousarray(a, np.uint8).reshape(32)
        b = np.ascontiguousarray(b, np.uint8).reshape(32)
        return check(lib().orbhip_descriptor_distance(ptr(a), ptr(b)), "DescriptorDistance")

    def match_bf(self, q_desc, q_angle, t_desc, t_angle, th_low: int | None = None):
        """Returns (nmatches, match[nq] (train idx or -1), best[nq], second[nq])."""
        q = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t_desc, np.uint8).reshape(-1, 32)
        qa = np.ascontiguousarray(q_angle, np.float32).reshape(-1)
        ta = np.ascontiguousarray(t_angle, np.float32).reshape(-1)
        nq, nt = q.shape[0], t.shape[0]
        m = np.full(nq, -1, np.int32); b = np.zeros(nq, np.int32); s = np.zeros(nq, np.int32)
        th = self.TH_LOW if th_low is None else int(th_low)
        n = lib().orbhip_match_bf(self.ctx.handle, ptr(q), ptr(qa), nq, ptr(t), ptr(ta), nt, th,
                                  ctypes.c_float(self.mfNNratio), int(self.mbCheckOrientation),
                                  ptr(m), ptr(b), ptr(s))
        return check(n, "orbhip_match_bf"), m, b, s

    def match_pairs_device(self, kps, desc, n, match, best, second, nmatch, th_low=None, stream=None):
        """Device tensors from ORBextractor.extract_batch_device: match frame p -> p+1."""
        B, cap = desc.shape[0], desc.shape[1]
        th = self.TH_LOW if th_low is None else int(th_low)
        st = torch_stream(stream)
        check(lib().orbhip_match_pairs_device(self.ctx.handle, ptr(kps), ptr(desc), ptr(n), B, cap, th,
                                              ctypes.c_float(self.mfNNratio), int(self.mbCheckOrientation),
                                              ptr(match), ptr(best), ptr(second), ptr(nmatch), st),
              "orbhip_match_pairs_device")

    def match_frames_device(self, q_kps, q_desc, nq, t_kps, t_desc, nt, match, best, second, nmatch, th_low=None,
                            stream=None):
        """Device tensors of two frames in separate allocations: kps (cap, 6) float32, desc (cap, 32)
        uint8, nq / nt int32 device scalars; match / best / second (cap,) int32, nmatch (1,) int32."""
        cap = q_desc.shape[0]
        if t_desc.shape[0] != cap:
            raise ValueError("match_frames_device: query and train capacities differ")
        th = self.TH_LOW if th_low is None else int(th_low)
        st = torch_stream(stream)
        check(lib().orbhip_match_frames_device(self.ctx.handle, ptr(q_kps), ptr(q_desc), ptr(nq), ptr(t_kps),
                                               ptr(t_desc), ptr(nt), cap, th, ctypes.c_float(self.mfNNratio),
                                               int(self.mbCheckOrientation), ptr(match), ptr(best), ptr(second),
                                               ptr(nmatch), st), "orbhip_match_frames_device")

    def SearchByBoW(self, kf_desc, kf_angle, kf_node, kf_weight, kf_valid, f_desc, f_angle, f_node, f_weight,
                    th_low: int | None = None):
        """U:src/ORBmatcher.cc::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) on the GPU.
        node / weight come from ORBVocabulary.transform_features (FeatureVector = weight > 0);
        kf_valid[i]: the KF feature has a good map point. Returns (nmatches, match[nf]) with
        match[f] = KF feature index (its MapPoint in the reference) or -1."""
        c = np.ascontiguousarray
        kd, fd = c(kf_desc, np.uint8).reshape(-1, 32), c(f_desc, np.uint8).reshape(-1, 32)
        ka, fa = c(kf_angle, np.float32), c(f_angle, np.float32)
        kn, fn = c(kf_node, np.int32), c(f_node, np.int32)
        kw, fw = c(kf_weight, np.float64), c(f_weight, np.float64)
        kv = c(kf_valid, np.uint8)
        nkf, nf = kd.shape[0], fd.shape[0]
        m = np.full(nf, -1, np.int32)
        th = self.TH_LOW if th_low is None else int(th_low)
        n = check(lib().orbhip_search_bow(self.ctx.handle, ptr(kd), ptr(ka), ptr(kn), ptr(kw), ptr(kv), nkf, ptr(fd),
                                          ptr(fa), ptr(fn), ptr(fw), nf, ctypes.c_float(self.mfNNratio),
                                          int(self.mbCheckOrientation), th, ptr(m)), "orbhip_search_bow")
        return n, m

    def SearchForInitialization(self, kps1, desc1, kps2, desc2, vbPrevMatched, windowSize: int = 10,
                                bounds2=(0.0, 640.0, 0.0, 480.0)):
        """U:src/ORBmatcher.cc::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)
        with the exact greedy semantics (Tracking::MonocularInitialization uses ORBmatcher(0.9, true)
        and windowSize 100). kps: orbhip_kp records; bounds2 = F2's (mnMinX, mnMaxX, mnMinY, mnMaxY).
        Returns (nmatches, vnMatches12, vbPrevMatched updated for the matches)."""
        k1 = np.ascontiguousarray(kps1, KP_DTYPE); k2 = np.ascontiguousarray(kps2, KP_DTYPE)
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        prev = np.ascontiguousarray(vbPrevMatched, np.float32).reshape(-1, 2).copy()
        m = np.full(k1.shape[0], -1, np.int32)
        f1 = InitFrameC(k1.shape[0], ptr(k1), ptr(d1), 0.0, 1.0, 0.0, 1.0)
        f2 = InitFrameC(k2.shape[0], ptr(k2), ptr(d2), *[float(b) for b in bounds2])
        n = check(lib().orbhip_search_for_initialization(self.ctx.handle, ctypes.byref(f1), ctypes.byref(f2),
                                                         ptr(prev), int(windowSize), ctypes.c_float(self.mfNNratio),
                                                         int(self.mbCheckOrientation), ptr(m)),
                  "orbhip_search_for_initialization")
        return n, m, prev

    # ---- projection-guided matching ----
    def SearchByProjectionLastFrame(self, frame: "ProjFrame", points, mp_desc, last_octave, last_angle,
                                    th: float = 15.0, last_pose=None):
        """U:src/ORBmatcher.cc::SearchByProjection(CurrentFrame, LastFrame, th, bMono).
        Queries = LastFrame entries with a non-outlier MapPoint (index order). Returns
        (nmatches, match[q] = CurrentFrame keypoint or -1). A frame that carries u_right takes the
        stereo branch (bMono = false): last_pose = (q, t) of LastFrame.GetPose() is then required, the
        level window follows the direction of motion and candidates are gated on their right
        coordinate; the direction found (1 forward, -1 backward, 0 neither) is left in
        self.last_direction."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        oc = np.ascontiguousarray(last_octave, np.int32)
        an = np.ascontiguousarray(last_angle, np.float32)
        match = np.empty(pts.shape[0], np.int32)   # written in full by the call
        lc = ProjLastC(pts.shape[0], ptr(pts), ptr(d), ptr(oc), ptr(an))
        if frame.u_right is not None:
            if last_pose is None:
                raise ValueError("SearchByProjectionLastFrame: a stereo frame needs last_pose = (q, t) of the last frame")
            lq = np.ascontiguousarray(last_pose[0], np.float32).reshape(4)
            lt = np.ascontiguousarray(last_pose[1], np.float32).reshape(3)
            sc = frame.to_c_stereo()
            direction = ctypes.c_int32(0)
            n = check(lib().orbhip_search_by_projection_last_stereo(self.ctx.handle, ctypes.byref(sc), ctypes.byref(lc),
                                                                    ptr(lq), ptr(lt), float(th),
                                                                    int(self.mbCheckOrientation), ptr(match),
                                                                    ctypes.byref(direction)),
                      "orbhip_search_by_projection_last_stereo")
            self.last_direction = int(direction.value)
            return n, match
        fc = frame.to_c()
        n = check(lib().orbhip_search_by_projection_last(self.ctx.handle, ctypes.byref(fc), ctypes.byref(lc),
                                                         float(th), int(self.mbCheckOrientation), ptr(match)),
                  "orbhip_search_by_projection_last")
        return n, match

    def SearchLocalPoints(self, frame: "ProjFrame", points, normals, min_dist, max_dist, mp_desc, skip=None,
                          th: float = 1.0, view_cos_limit: float = 0.5, far_points: bool = False,
                          th_far: float = 0.0):
        """Tracking::SearchLocalPoints: Frame::isInFrustum + SearchByProjection(F, vpMapPoints, th,
        bFarPoints, thFarPoints) with this matcher's nnratio. Returns (nmatches, match, in_view, level).
        A frame that carries u_right takes the stereo branch (candidates gated on their right
        coordinate) and also returns proj_xr (mTrackProjXR where in_view, NaN elsewhere)."""
        key = (id(points), id(normals), id(min_dist), id(max_dist), id(mp_desc), id(skip))
        hit = self._lp_cache
        if hit is not None and hit[0] == key and all(a is b for a, b in zip(hit[1], (points, normals, min_dist,
                                                                                      max_dist, mp_desc, skip))):
            lc, m = hit[2], hit[3]   # the same arrays as the last call: their C view is still valid
        else:
            pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
            nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            mn = np.ascontiguousarray(min_dist, np.float32)
            mx = np.ascontiguousarray(max_dist, np.float32)
            d = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
            sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
            m = pts.shape[0]
            lc = LocalPointsC(m, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(d), ptr(sk))
            # cached only when no conversion copied an input (the view then reads the caller's
            # memory, so in-place updates are seen); the inputs live with it, so their ids stay theirs
            srcs = (points, normals, min_dist, max_dist, mp_desc, skip)
            views = (pts, nrm, mn, mx, d, sk)
            zero_copy = all(v is o or (v is not None and v.base is o) for v, o in zip(views, srcs))
            self._lp_cache = (key, srcs, lc, m, views) if zero_copy else None
        match = np.empty(m, np.int32)      # written in full by the call (m > 0)
        in_view = np.empty(m, np.uint8)
        level = np.empty(m, np.int32)
        if frame.u_right is not None:
            proj_xr = np.full(m, np.nan, np.float32)
            sc = frame.to_c_stereo()
            n = check(lib().orbhip_search_local_points_stereo(self.ctx.handle, ctypes.byref(sc), ctypes.byref(lc),
                                                              float(view_cos_limit), float(th), float(self.mfNNratio),
                                                              int(far_points), float(th_far), ptr(in_view), ptr(level),
                                                              ptr(proj_xr), ptr(match)),
                      "orbhip_search_local_points_stereo")
            return n, match, in_view, level, proj_xr
        fc = frame.to_c()
        n = check(lib().orbhip_search_local_points(self.ctx.handle, ctypes.byref(fc), ctypes.byref(lc),
                                                   float(view_cos_limit), float(th), float(self.mfNNratio),
                                                   int(far_points), float(th_far), ptr(in_view), ptr(level),
                                                   ptr(match)), "orbhip_search_local_points")
        return n, match, in_view, level

    # ---- new map points (LocalMapping::CreateNewMapPoints) ----
    def SearchForTriangulation(self, kf1: "TriKeyFrame", neighbours, scale_factors, level_sigma2):
        """U:src/ORBmatcher.cc::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, false, false) of
        kf1 against every keyframe of `neighbours` (at most 64) in one call, with this matcher's
        mbCheckOrientation (CreateNewMapPoints uses ORBmatcher(0.6, false); there is no ratio test).
        Returns (nmatches[B], match12[B, n1]) with match12[b, i] = the feature of neighbour b
        matched to kf1's feature i, or -1. Keyframes that carry u_right take the stereo branch (no
        epipole exclusion for a pair with a stereo feature); all keyframes of a call must agree."""
        nb = list(neighbours)
        B, n1 = len(nb), kf1.n
        stereo = _tri_stereo("SearchForTriangulation", kf1, nb)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        if sf.shape[0] != s2.shape[0]:
            raise ValueError("SearchForTriangulation: scale_factors and level_sigma2 differ in length")
        nm = np.zeros(B, np.int32)
        m = np.full((B, n1), -1, np.int32)
        if B == 0:
            return nm, m
        if stereo:
            arr = (TriStereoKeyFrameC * B)(*[k.to_c_stereo() for k in nb])
            c1 = kf1.to_c_stereo()
            check(lib().orbhip_search_for_triangulation_stereo(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(sf),
                                                               ptr(s2), sf.shape[0], int(self.mbCheckOrientation),
                                                               ptr(m), ptr(nm)),
                  "orbhip_search_for_triangulation_stereo")
            return nm, m
        arr = (TriKeyFrameC * B)(*[k.to_c() for k in nb])
        c1 = kf1.to_c()
        check(lib().orbhip_search_for_triangulation(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(sf), ptr(s2),
                                                    sf.shape[0], int(self.mbCheckOrientation), ptr(m), ptr(nm)),
              "orbhip_search_for_triangulation")
        return nm, m

    def CreateNewMapPoints(self, kf1: "TriKeyFrame", neighbours, scale_factors, level_sigma2, median_depth=None,
                           cos_parallax_max: float = 0.9998, ratio_factor=None, far_threshold: float = 0.0,
                           diagnostics: bool = False) -> "NewPoints":
        """SearchForTriangulation of kf1 against every neighbour and the triangulation and checks of
        U:src/LocalMapping.cc::CreateNewMapPoints on its matches, in one call (orbhip_create_new_map_points).
        median_depth: per neighbour its ComputeSceneMedianDepth(2), or None (no neighbour is gated);
        ratio_factor: None = 1.5f * mvScaleFactors[1]; far_threshold <= 0: off. diagnostics: also
        return match12, status and x3d_all (B x n1). Keyframes that carry u_right (all of a call or
        none) take the stereo branch (orbhip_create_new_map_points_stereo): a neighbour is gated when
        the baseline is below its b, median_depth must be None, and diagnostics include `source`."""
        return self._new_points("orbhip_create_new_map_points", kf1, neighbours, scale_factors, level_sigma2, None,
                                median_depth, cos_parallax_max, ratio_factor, far_threshold, diagnostics)

    def TriangulateMatches(self, kf1: "TriKeyFrame", neighbours, match12, scale_factors, level_sigma2,
                           cos_parallax_max: float = 0.9998, ratio_factor=None, far_threshold: float = 0.0,
                           diagnostics: bool = False) -> "NewPoints":
        """The triangulation and checks of CreateNewMapPoints on given matches (match12: B x n1, a
        neighbour feature or -1): no search, no gating (orbhip_triangulate_matches)."""
        return self._new_points("orbhip_triangulate_matches", kf1, neighbours, scale_factors, level_sigma2, match12,
                                None, cos_parallax_max, ratio_factor, far_threshold, diagnostics)

    def _new_points(self, what, kf1, neighbours, scale_factors, level_sigma2, match12, median_depth, cos_parallax_max,
                    ratio_factor, far_threshold, diagnostics):
        nb = list(neighbours)
        B, n1 = len(nb), kf1.n
        stereo = _tri_stereo(what, kf1, nb)
        if stereo and median_depth is not None:
            raise ValueError(f"{what}: stereo keyframes are gated on their b, not on median_depth")
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        if sf.shape[0] != s2.shape[0]:
            raise ValueError(f"{what}: scale_factors and level_sigma2 differ in length")
        if ratio_factor is None:
            ratio_factor = np.float32(1.5) * sf[1]
        prm = TriParamsC(float(cos_parallax_max), float(np.float32(ratio_factor)), float(np.float32(far_threshold)))
        r = NewPoints(B, n1, diagnostics, stereo)
        out = NewPointsC(ptr(r.match12), ptr(r.nmatches), ptr(r.gated), ptr(r.status), ptr(r.x3d_all), ptr(r.first),
                         ptr(r.nnew), ptr(r._nbr), ptr(r._idx1), ptr(r._idx2), ptr(r._x3d))
        if stereo:
            arr = (TriStereoKeyFrameC * max(B, 1))(*[k.to_c_stereo() for k in nb])
            c1 = kf1.to_c_stereo()
            if match12 is None:
                n = lib().orbhip_create_new_map_points_stereo(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(sf), ptr(s2),
                                                              sf.shape[0], int(self.mbCheckOrientation),
                                                              ctypes.byref(prm), ctypes.byref(out), ptr(r.source))
            else:
                m = np.ascontiguousarray(match12, np.int32)
                if m.shape != (B, n1):
                    raise ValueError(f"{what}: match12 must be B x n1")
                n = lib().orbhip_triangulate_matches_stereo(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(m), ptr(sf),
                                                            ptr(s2), sf.shape[0], ctypes.byref(prm), ctypes.byref(out),
                                                            ptr(r.source))
            r.n = check(n, what + "_stereo")
            return r
        arr = (TriKeyFrameC * max(B, 1))(*[k.to_c() for k in nb])
        c1 = kf1.to_c()
        if match12 is None:
            md = None
            if median_depth is not None:
                md = np.ascontiguousarray(median_depth, np.float32)
                if md.shape != (B,):
                    raise ValueError(f"{what}: median_depth needs one value per neighbour")
            n = lib().orbhip_create_new_map_points(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(md), ptr(sf), ptr(s2),
                                                   sf.shape[0], int(self.mbCheckOrientation), ctypes.byref(prm),
                                                   ctypes.byref(out))
        else:
            m = np.ascontiguousarray(match12, np.int32)
            if m.shape != (B, n1):
                raise ValueError(f"{what}: match12 must be B x n1")
            n = lib().orbhip_triangulate_matches(self.ctx.handle, ctypes.byref(c1), arr, B, ptr(m), ptr(sf), ptr(s2),
                                                 sf.shape[0], ctypes.byref(prm), ctypes.byref(out))
        r.n = check(n, what)
        return r

    # ---- map point fusion (LocalMapping::SearchInNeighbors) ----
    def Fuse(self, kfs, points, normals, min_dist, max_dist, mp_desc, inv_level_sigma2, th: float = 3.0,
             skip=None, pair_skip=None):
        """U:src/ORBmatcher.cc::Fuse(pKF, vpMapPoints, th) of every keyframe of `kfs` (a list of
        ProjFrame, at most 64, one scale pyramid) against the same MapPoints in one call.
        skip[m] = !pMP || isBad(), pair_skip[b, m] = pMP->IsInKeyFrame(kfs[b]). Every point is seen as
        it is at call time; the caller applies Replace / AddObservation / AddMapPoint in upstream
        order. Returns (nfused[B], best_idx[B, n], best_dist[B, n], level[B, n]):
        best_idx = the keypoint of kfs[b] the point fuses into or -1, best_dist = the least distance
        over the gated candidates (256: none), level = nPredictedLevel (-1: rejected before it).
        Keyframes that carry u_right take the stereo branch (orbhip_fuse_stereo: a candidate with
        u_right >= 0 is gated on its right coordinate too, at 7.8); all keyframes of a call must
        agree, else ValueError."""
        kfs = list(kfs)
        B = len(kfs)
        stereo = B > 0 and kfs[0].u_right is not None
        if any((k.u_right is not None) != stereo for k in kfs):
            raise ValueError("Fuse: stereo and monocular keyframes in one call")
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        mn = np.ascontiguousarray(min_dist, np.float32)
        mx = np.ascontiguousarray(max_dist, np.float32)
        d = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        ps = None if pair_skip is None else np.ascontiguousarray(pair_skip, np.uint8).reshape(B, n)
        s2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        for a in (nrm, mn, mx, d) + (() if sk is None else (sk,)):
            if a.shape[0] != n:
                raise ValueError("Fuse: per-point arrays differ in length")
        nf = np.zeros(B, np.int32)
        idx = np.full((B, n), -1, np.int32)
        dist = np.full((B, n), 256, np.int32)
        lvl = np.full((B, n), -1, np.int32)
        if B == 0:
            return nf, idx, dist, lvl
        if any(s2.shape[0] < len(k.scale_factors) for k in kfs):
            raise ValueError("Fuse: inv_level_sigma2 shorter than the keyframes' scale tables")
        lc = LocalPointsC(n, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(d), ptr(sk))
        if stereo:
            views = (StereoViewC * B)(*[k.to_c_stereo() for k in kfs])
            check(lib().orbhip_fuse_stereo(self.ctx.handle, views, B, ctypes.byref(lc), ptr(ps), ptr(s2), float(th),
                                           ptr(idx), ptr(dist), ptr(lvl), ptr(nf)), "orbhip_fuse_stereo")
            return nf, idx, dist, lvl
        arr = (FrameC * B)(*[k.to_c() for k in kfs])
        check(lib().orbhip_fuse(self.ctx.handle, arr, B, ctypes.byref(lc), ptr(ps), ptr(s2), float(th), ptr(idx),
                                ptr(dist), ptr(lvl), ptr(nf)), "orbhip_fuse")
        return nf, idx, dist, lvl

    # ---- loop closing (LoopClosing::SearchAndFuse, DetectCommonRegionsFromBoW, ...) ----
    @staticmethod
    def _points_c(what, points, normals, min_dist, max_dist, mp_desc, skip):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        mn = np.ascontiguousarray(min_dist, np.float32)
        mx = np.ascontiguousarray(max_dist, np.float32)
        d = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        for a in (nrm, mn, mx, d) + (() if sk is None else (sk,)):
            if a.shape[0] != n:
                raise ValueError(f"{what}: per-point arrays differ in length")
        # (the arrays are returned with the view: it points into them)
        return n, LocalPointsC(n, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(d), ptr(sk)), (pts, nrm, mn, mx, d, sk)

    def FuseSim3(self, kfs, points, normals, min_dist, max_dist, mp_desc, th: float = 4.0, skip=None,
                 pair_skip=None):
        """U:src/ORBmatcher.cc::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of every keyframe of `kfs`
        against the same MapPoints in one call (LoopClosing::SearchAndFuse, th = 4). Each ProjFrame
        carries Tcw = (Scw.rotationMatrix(), Scw.translation() / Scw.scale()). The rule of Fuse
        without the chi-square gate; skip[m] = isBad(), pair_skip[b, m] = the keyframe already holds
        the point. Returns (nfused[B], best_idx[B, n], best_dist[B, n], level[B, n]) as Fuse."""
        kfs = list(kfs)
        B = len(kfs)
        n, lc, keep = self._points_c("FuseSim3", points, normals, min_dist, max_dist, mp_desc, skip)
        ps = None if pair_skip is None else np.ascontiguousarray(pair_skip, np.uint8).reshape(B, n)
        nf = np.zeros(B, np.int32)
        idx = np.full((B, n), -1, np.int32)
        dist = np.full((B, n), 256, np.int32)
        lvl = np.full((B, n), -1, np.int32)
        if B == 0:
            return nf, idx, dist, lvl
        arr = (FrameC * B)(*[k.to_c() for k in kfs])
        check(lib().orbhip_fuse_sim3(self.ctx.handle, arr, B, ctypes.byref(lc), ptr(ps), float(th), ptr(idx),
                                     ptr(dist), ptr(lvl), ptr(nf)), "orbhip_fuse_sim3")
        return nf, idx, dist, lvl

    def SearchByProjectionSim3(self, kf: "ProjFrame", points, normals, min_dist, max_dist, mp_desc, th: float,
                               ratioHamming: float = 1.0, skip=None):
        """U:src/ORBmatcher.cc::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming)
        (and the overload with vpPointsKFs / vpMatchedKF) with upstream's sequential greedy semantics.
        kf carries Tcw = (R, t / s) of Scw and claimed[k] = vpMatched[k] is set at call time;
        skip[m] = isBad() or the point is in vpMatched already. Returns (nmatches, match[n] = the
        keypoint the point claims or -1, match_dist[n] = its distance or 256, level[n])."""
        n, lc, keep = self._points_c("SearchByProjectionSim3", points, normals, min_dist, max_dist, mp_desc, skip)
        match = np.full(n, -1, np.int32)
        dist = np.full(n, 256, np.int32)
        lvl = np.full(n, -1, np.int32)
        fc = kf.to_c()
        nm = check(lib().orbhip_search_by_projection_sim3(self.ctx.handle, ctypes.byref(fc), ctypes.byref(lc), float(th),
                                                          float(ratioHamming), ptr(match), ptr(dist), ptr(lvl)),
                   "orbhip_search_by_projection_sim3")
        return nm, match, dist, lvl


def _tri_stereo(what, kf1, nb) -> bool:
    """Whether the keyframes of a triangulation call are stereo (all or none, else ValueError)."""
    stereo = kf1.u_right is not None
    if any((k.u_right is not None) != stereo for k in nb):
        raise ValueError(f"{what}: stereo and monocular keyframes in one call")
    return stereo


class NewPoints:
    """What CreateNewMapPoints / TriangulateMatches return. n new points, in upstream's creation
    order (ascending neighbour, then ascending idx1): new_nbr, new_idx1, new_idx2, new_x3d (views of
    the first n entries). first[idx1] = the neighbour whose point the feature became or -1;
    nnew[b], nmatches[b], gated[b] per neighbour. With diagnostics: match12, status and x3d_all
    (B x n1; status codes in include/orbhip.h), else None; a stereo call's diagnostics also hold
    source (B x n1: 0 no point, 1 triangulated, 2 / 3 unprojected from KF1 / the neighbour)."""

    def __init__(self, B: int, n1: int, diagnostics: bool, stereo: bool = False):
        self.n = 0
        self.nmatches = np.zeros(B, np.int32)
        self.gated = np.zeros(B, np.uint8)
        self.first = np.full(n1, -1, np.int32)
        self.nnew = np.zeros(B, np.int32)
        self._nbr = np.full(n1, -1, np.int32)
        self._idx1 = np.full(n1, -1, np.int32)
        self._idx2 = np.full(n1, -1, np.int32)
        self._x3d = np.zeros((n1, 3), np.float32)
        self.match12 = np.full((B, n1), -1, np.int32) if diagnostics else None
        self.status = np.zeros((B, n1), np.uint8) if diagnostics else None
        self.x3d_all = np.zeros((B, n1, 3), np.float32) if diagnostics else None
        self.source = np.zeros((B, n1), np.uint8) if diagnostics and stereo else None

    new_nbr = property(lambda self: self._nbr[:self.n])
    new_idx1 = property(lambda self: self._idx1[:self.n])
    new_idx2 = property(lambda self: self._idx2[:self.n])
    new_x3d = property(lambda self: self._x3d[:self.n])


class TriKeyFrame:
    """A KeyFrame as SearchForTriangulation reads it: mvKeysUn (orbhip_kp records), descriptors, the
    FeatureVector as per-feature (node, weight) from ORBVocabulary.transform_features (levelsup 4;
    weight > 0 and node >= 0: in the vector), has_mp[i] = GetMapPoint(i) is set, the pinhole
    intrinsics and Tcw. A rectified-stereo keyframe also carries u_right (mvuRight) and depth (mvDepth),
    one per feature, bf (mbf) and b (mb); the calls then take their stereo branches."""

    def __init__(self, kps, desc, node, weight, has_mp, pose_q, pose_t, fx, fy, cx, cy, u_right=None, depth=None,
                 bf=0.0, b=0.0):
        self.kps = np.ascontiguousarray(kps, KP_DTYPE)
        self.n = self.kps.shape[0]
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.node = np.ascontiguousarray(node, np.int32)
        self.weight = np.ascontiguousarray(weight, np.float64)
        self.has_mp = np.ascontiguousarray(has_mp, np.uint8)
        for a in (self.desc, self.node, self.weight, self.has_mp):
            if a.shape[0] != self.n:
                raise ValueError("TriKeyFrame: per-feature arrays differ in length")
        self.pose_q = np.array(pose_q, np.float32).reshape(4)
        self.pose_t = np.array(pose_t, np.float32).reshape(3)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self._c = None
        if (u_right is None) != (depth is None):
            raise ValueError("TriKeyFrame: u_right and depth come together")
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, np.float32).reshape(-1)
        self.depth = None if depth is None else np.ascontiguousarray(depth, np.float32).reshape(-1)
        self.bf, self.b = float(bf), float(b)

    def to_c_stereo(self) -> TriStereoKeyFrameC:
        """The stereo view: to_c() plus u_right / depth / bf / b (it points into this object's arrays)."""
        self.u_right = np.ascontiguousarray(self.u_right, np.float32).reshape(-1)
        self.depth = np.ascontiguousarray(self.depth, np.float32).reshape(-1)
        c = TriStereoKeyFrameC()
        c.kf = self.to_c()
        if self.u_right.shape[0] != self.n or self.depth.shape[0] != self.n:
            raise ValueError("TriKeyFrame: u_right and depth need one entry per feature")
        c.u_right, c.depth, c.bf, c.b = ptr(self.u_right), ptr(self.depth), self.bf, self.b
        return c

    def to_c(self) -> TriKeyFrameC:
        """The C view (it points into this object's arrays: keep the object alive while it is used).
        The pointer fields are cached while the five per-feature arrays are the same objects (a
        neighbour list is passed again for every new keyframe); the pose and the intrinsics are
        re-filled on every call, so they may change in place or be reassigned."""
        hit = self._c
        if hit is None or not (hit[0][0] is self.kps and hit[0][1] is self.desc and hit[0][2] is self.node
                               and hit[0][3] is self.weight and hit[0][4] is self.has_mp):
            self.kps = np.ascontiguousarray(self.kps, KP_DTYPE)
            self.n = self.kps.shape[0]
            self.desc = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
            self.node = np.ascontiguousarray(self.node, np.int32)
            self.weight = np.ascontiguousarray(self.weight, np.float64)
            self.has_mp = np.ascontiguousarray(self.has_mp, np.uint8)
            arrs = (self.kps, self.desc, self.node, self.weight, self.has_mp)
            if any(a.shape[0] != self.n for a in arrs):
                raise ValueError("TriKeyFrame: per-feature arrays differ in length")
            c = TriKeyFrameC()
            c.n = self.n
            c.kps, c.desc, c.node, c.weight, c.has_mp = (ptr(a) for a in arrs)
            self._c = hit = (arrs, c)
        c = hit[1]
        c.fx, c.fy, c.cx, c.cy = self.fx, self.fy, self.cx, self.cy
        # (through float32 first: the C fields hold exactly what the arrays hold)
        c.pose_q[:] = np.asarray(self.pose_q, np.float32).reshape(4).tolist()
        c.pose_t[:] = np.asarray(self.pose_t, np.float32).reshape(3).tolist()
        return c

    def geometry(self, other: "TriKeyFrame"):
        """(F12 (3, 3), ep (2,)) of the pair (self = KF1, other = KF2), as the kernel consumes them
        (orbhip_triangulation_geometry: host only, fp32)."""
        F = np.zeros(9, np.float32)
        ep = np.zeros(2, np.float32)
        a, b = self.to_c(), other.to_c()
        check(lib().orbhip_triangulation_geometry(ctypes.byref(a), ctypes.byref(b), ptr(F), ptr(ep)),
              "orbhip_triangulation_geometry")
        return F.reshape(3, 3), ep


class ProjFrame:
    """The current Frame for projection matching (U:src/Frame.cc): keypoints (orbhip_kp records:
    mvKeysUn — PinholeCamera.UndistortKeyPoints for a distorted camera, mvKeys otherwise),
    descriptors, claimed mask, image bounds (Frame::ComputeImageBounds: PinholeCamera
    .ComputeImageBounds, or [0, width] x [0, height] without distortion), scale tables,
    intrinsics and Tcw. A rectified-stereo Frame also carries u_right (mvuRight, one per keypoint),
    bf (mbf) and b (mb); the searches then take their stereo branches."""

    def __init__(self, kps, desc, pose_q, pose_t, fx, fy, cx, cy, width=640, height=480, scale_factor=1.2,
                 n_levels=8, claimed=None, bounds=None, u_right=None, bf=0.0, b=0.0):
        self.kps = np.ascontiguousarray(kps, KP_DTYPE)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.claimed = None if claimed is None else np.ascontiguousarray(claimed, np.uint8)
        self.pose_q = np.asarray(pose_q, np.float32).reshape(4)
        self.pose_t = np.asarray(pose_t, np.float32).reshape(3)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)
        self.bounds = (0.0, float(width), 0.0, float(height)) if bounds is None else tuple(float(b) for b in bounds)
        sf = np.ones(n_levels, np.float32)
        for i in range(1, n_levels):
            sf[i] = np.float32(np.float64(sf[i - 1]) * np.float64(np.float32(scale_factor)))
        self.scale_factors = sf
        self.log_scale_factor = float(np.log(np.float32(scale_factor)).astype(np.float32))
        self._c = self._cs = None
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, np.float32).reshape(-1)
        self.bf, self.b = float(bf), float(b)

    def to_c_stereo(self) -> StereoViewC:
        """The stereo view: to_c() plus u_right / bf / b. The u_right pointer is cached while
        u_right is the same array object (as to_c caches its arrays); the frame, bf and b are
        re-filled on every call."""
        hit = self._cs
        if hit is None or hit[0] is not self.u_right:
            self.u_right = np.ascontiguousarray(self.u_right, np.float32).reshape(-1)
            c = StereoViewC()
            c.u_right = ptr(self.u_right)
            self._cs = hit = (self.u_right, c)   # the view keeps the array it points into alive
        c = hit[1]
        c.frame = self.to_c()
        if hit[0].shape[0] != c.frame.n:
            raise ValueError("ProjFrame.u_right needs one entry per keypoint")
        c.bf, c.b = self.bf, self.b
        return c

    def to_c(self) -> FrameC:
        """The C view. The pointer fields are cached while kps / desc / claimed / scale_factors are
        the same array objects (Tracking keeps them between SearchByProjection and
        SearchLocalPoints); a reassigned array is converted again and its pointer refreshed. The
        scalars (pose, bounds, intrinsics) are re-filled on every call: Tcw changes in place after
        PoseOptimization."""
        arrs = (self.kps, self.desc, self.claimed, self.scale_factors)
        hit = self._c
        if hit is None or any(a is not b for a, b in zip(hit[0], arrs)):
            self.kps = np.ascontiguousarray(self.kps, KP_DTYPE)
            self.desc = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
            if self.claimed is not None:
                self.claimed = np.ascontiguousarray(self.claimed, np.uint8)
            self.scale_factors = np.ascontiguousarray(self.scale_factors, np.float32)
            c = FrameC()
            c.n = self.kps.shape[0]
            c.kps, c.desc, c.claimed = ptr(self.kps), ptr(self.desc), ptr(self.claimed)
            c.scale_factors, c.n_levels = ptr(self.scale_factors), len(self.scale_factors)
            # the view keeps the arrays it points into alive
            self._c = hit = ((self.kps, self.desc, self.claimed, self.scale_factors), c)
        c = hit[1]
        if self.claimed is not None and self.claimed.shape[0] < c.n:
            raise ValueError("ProjFrame.claimed shorter than kps")
        c.min_x, c.max_x, c.min_y, c.max_y = (float(b) for b in self.bounds)
        c.log_scale_factor = float(self.log_scale_factor)
        c.fx, c.fy, c.cx, c.cy = float(self.fx), float(self.fy), float(self.cx), float(self.cy)
        c.pose_q[:] = [float(v) for v in np.asarray(self.pose_q, np.float32).reshape(4)]
        c.pose_t[:] = [float(v) for v in np.asarray(self.pose_t, np.float32).reshape(3)]
        return c
