"""TwoViewReconstruction (U:src/TwoViewReconstruction.cc): the homography and fundamental-matrix
RANSAC of monocular initialisation, the model choice, the motion hypotheses and their CheckRT, every
pair of a batch in one device call (orbhip_two_view_reconstruct_batch, DESIGN.md
"TwoViewReconstruction").

The library draws no random numbers: the caller passes the 8-sets (``draw_sets`` restates upstream's
draw)."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._lib import KP_DTYPE, Context, TwoViewProblemC, TwoViewResultC, check, lib, ptr

MAX_BATCH, MAX_MATCHES, MAX_HYP = 64, 8192, 4096


def draw_sets(N: int, H: int, randint) -> np.ndarray:
    """H sets of 8 distinct indices in [0, N) as upstream draws them: from a fresh vAvailableIndices
    per iteration, eight times randi = randint(0, size - 1) (both ends included,
    DUtils::Random::RandomInt), take avail[randi], then avail[randi] = avail.back(); pop_back()."""
    if N < 8:
        raise ValueError("draw_sets needs N >= 8")
    out = np.empty((H, 8), np.int32)
    for h in range(H):
        avail = list(range(N))
        for k in range(8):
            r = int(randint(0, len(avail) - 1))
            out[h, k] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def _keys(keys) -> np.ndarray:
    """Keypoints as the library's records: a KP_DTYPE array as it is, or n x 2 coordinates."""
    if isinstance(keys, np.ndarray) and keys.dtype == KP_DTYPE:
        return np.ascontiguousarray(keys)
    xy = np.asarray(keys, np.float32)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("keypoints are a KP_DTYPE array or n x 2 coordinates")
    k = np.zeros(xy.shape[0], KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


class TwoViewReconstruction:
    """Upstream's class: K as (fx, fy, cx, cy), a 3 x 3 matrix or a camera with those members;
    sigma and iterations as upstream's constructor takes them."""

    def __init__(self, K, sigma: float = 1.0, iterations: int = 200, ctx: Context | None = None):
        if hasattr(K, "fx"):
            K = [K.fx, K.fy, K.cx, K.cy]
        K = np.asarray(K, np.float32)
        if K.shape == (3, 3):
            K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32)
        if K.shape != (4,):
            raise ValueError("K is (fx, fy, cx, cy) or a 3 x 3 matrix")
        if not (np.isfinite(K).all() and K[0] > 0 and K[1] > 0):
            raise ValueError("the focal lengths must be positive and finite")
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError("sigma must be positive and finite")
        if not 1 <= int(iterations) <= MAX_HYP:
            raise ValueError(f"iterations must lie in [1, {MAX_HYP}]")
        self.K, self.mSigma, self.mMaxIterations, self.ctx = K, float(sigma), int(iterations), ctx
        self.last = None   # the diagnostics of the last Reconstruct

    def _problem(self, keys1, keys2, matches12, sets):
        k1, k2 = _keys(keys1), _keys(keys2)
        m = np.ascontiguousarray(matches12, np.int32)
        if m.shape != (k1.shape[0],):
            raise ValueError("vMatches12 holds one entry per keypoint of frame 1")
        if m.size and (m.min() < -1 or m.max() >= k2.shape[0]):
            raise ValueError("a match outside [-1, n2)")
        N = int((m >= 0).sum())
        if N < 8:
            raise ValueError("fewer than 8 matches")
        if N > MAX_MATCHES:
            raise ValueError(f"more than {MAX_MATCHES} matches")
        s = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        if s.shape[0] < self.mMaxIterations:
            raise ValueError(f"{s.shape[0]} sets for {self.mMaxIterations} iterations")
        s = np.ascontiguousarray(s[:self.mMaxIterations])
        srt = np.sort(s, 1)
        if s.min() < 0 or s.max() >= N or (srt[:, 1:] == srt[:, :-1]).any():
            raise ValueError("a set index outside [0, N) or repeated within its set")
        return k1, k2, m, s, N

    def Reconstruct(self, keys1, keys2, matches12, sets):
        """-> (ok, T21 4 x 4, vP3D n1 x 3, vbTriangulated n1)"""
        return TwoViewReconstruction.reconstruct_batch([self], [(keys1, keys2, matches12, sets)])[0]

    @staticmethod
    def reconstruct_batch(solvers, pairs):
        """Several frame pairs in one device call (up to 64): pairs[b] = (keys1, keys2, matches12,
        sets) -> one (ok, T21, vP3D, vbTriangulated) per pair."""
        if len(solvers) != len(pairs):
            raise ValueError("one frame pair per solver")
        B = len(solvers)
        if B == 0:
            return []
        if B > MAX_BATCH:
            raise ValueError(f"more than {MAX_BATCH} pairs in one call")
        preps = [s._problem(*p) for s, p in zip(solvers, pairs)]
        ctx = next((s.ctx for s in solvers if s.ctx is not None), None)
        if ctx is None:
            ctx = solvers[0].ctx = Context()
        probs, ress = (TwoViewProblemC * B)(), (TwoViewResultC * B)()
        outs = []
        for b, (s, (k1, k2, m, st, N)) in enumerate(zip(solvers, preps)):
            n1 = k1.shape[0]
            p3d, tri = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
            ih, jf = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
            probs[b] = TwoViewProblemC(n1, k2.shape[0], ptr(k1), ptr(k2), ptr(m), (ctypes.c_float * 4)(*s.K),
                                       s.mSigma, st.shape[0], ptr(st))
            ress[b].p3d, ress[b].triangulated, ress[b].inliers_h, ress[b].inliers_f = ptr(p3d), ptr(tri), ptr(ih), ptr(jf)
            outs.append((p3d, tri, ih, jf))
        check(lib().orbhip_two_view_reconstruct_batch(ctx.handle, probs, B, ress), "orbhip_two_view_reconstruct_batch")
        ret = []
        for b, s in enumerate(solvers):
            r, (p3d, tri, ih, jf) = ress[b], outs[b]
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = np.array(r.R21, np.float32).reshape(3, 3)
            T[:3, 3] = np.array(r.t21, np.float32)
            s.last = dict(success=int(r.success), model=int(r.model), best_h=int(r.best_h), best_f=int(r.best_f),
                          chosen=int(r.chosen), SH=np.float32(r.SH), SF=np.float32(r.SF),
                          H21=np.array(r.H21, np.float32).reshape(3, 3), F21=np.array(r.F21, np.float32).reshape(3, 3),
                          R21=T[:3, :3].copy(), t21=T[:3, 3].copy(), n_good=np.array(r.n_good, np.int32),
                          parallax=np.array(r.parallax, np.float32), cos_sel=np.array(r.cos_sel, np.float32),
                          inl_h=ih.astype(bool), inl_f=jf.astype(bool), p3d=p3d, triangulated=tri.astype(bool))
            ret.append((bool(r.success), T, p3d, tri.astype(bool)))
        return ret
