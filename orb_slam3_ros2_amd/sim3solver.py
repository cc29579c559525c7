"""Sim3Solver (U:src/Sim3Solver.cc): Horn's closed form on RANSAC triples, every hypothesis of every
candidate in one device call (orbhip_sim3_solve_batch, DESIGN.md "Sim3Solver").

The hypotheses are independent once their triples are drawn, so ``solve`` evaluates all
``mRansacMaxIts`` of them at once and ``iterate`` walks the stored counts with upstream's state: the
same matrices, flags and inliers as the sequential loop, chunk by chunk. The library draws no random
numbers: the caller passes the triples (``draw_triples`` restates upstream's draw)."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._lib import Context, Sim3ProblemC, Sim3ResultC, check, lib, ptr

HYP_FLOATS = 13   # (s, R row-major, t) per hypothesis


def error_bounds(octaves, level_sigma2) -> np.ndarray:
    """mvnMaxError: upstream stores 9.210 * sigma2[octave] in a vector<size_t>, so the bound is the
    product truncated to an integer: (float)(size_t)(9.210 * (double)sigma2)."""
    s2 = np.asarray(level_sigma2, np.float32).astype(np.float64)[np.asarray(octaves, np.int64)]
    return np.floor(9.210 * s2).astype(np.float32)


def draw_triples(N: int, H: int, randint) -> np.ndarray:
    """H triples of distinct indices in [0, N) as upstream draws them: from a fresh mvAllIndices per
    iteration, three times randi = randint(0, size - 1) (both ends included, DUtils::Random::RandomInt),
    take avail[randi], then avail[randi] = avail.back(); pop_back()."""
    if N < 3:
        raise ValueError("draw_triples needs N >= 3")
    out = np.empty((H, 3), np.int32)
    for h in range(H):
        avail = list(range(N))
        for k in range(3):
            r = int(randint(0, len(avail) - 1))
            out[h, k] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


def _cam4(cam) -> np.ndarray:
    c = np.asarray([getattr(cam, k) for k in ("fx", "fy", "cx", "cy")] if hasattr(cam, "fx") else cam, np.float32)
    if c.shape != (4,):
        raise ValueError("a camera is (fx, fy, cx, cy)")
    return c


class Sim3Solver:
    """Upstream's class state over the N correspondences the constructor's filter leaves.

    X1c / X2c: the map points in the frames of camera 1 / 2 (Rcw Xw + tcw), N x 3 float32;
    octaves1 / octaves2: the keypoints' octaves; level_sigma2_1 / _2: the keyframes' mvLevelSigma2;
    cam1 / cam2: (fx, fy, cx, cy); indices1: mvnIndices1 (keypoint index in keyframe 1 per
    correspondence, default 0..N-1) and n1: mN1, the length of iterate's vbInliers."""

    def __init__(self, X1c, X2c, octaves1, octaves2, level_sigma2_1, level_sigma2_2, cam1, cam2, fix_scale,
                 indices1=None, n1=None, ctx: Context | None = None):
        self.X1 = np.ascontiguousarray(X1c, np.float32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2c, np.float32).reshape(-1, 3)
        self.N = self.X1.shape[0]
        if self.X2.shape[0] != self.N:
            raise ValueError("X1c and X2c differ in length")
        self.max_err1 = error_bounds(octaves1, level_sigma2_1)
        self.max_err2 = error_bounds(octaves2, level_sigma2_2)
        if self.max_err1.shape != (self.N,) or self.max_err2.shape != (self.N,):
            raise ValueError("one octave per correspondence")
        self.cam1, self.cam2 = _cam4(cam1), _cam4(cam2)
        self.fix_scale = bool(fix_scale)
        self.indices1 = np.arange(self.N, dtype=np.int64) if indices1 is None else np.asarray(indices1, np.int64)
        self.n1 = int(self.N if n1 is None else n1)
        if self.indices1.shape != (self.N,) or (self.N and (self.indices1.min() < 0 or self.indices1.max() >= self.n1)):
            raise ValueError("indices1 must map every correspondence into [0, n1)")
        self.ctx = ctx
        self.mnBestInliers = 0
        self.mBestT12 = np.eye(4, dtype=np.float32)
        self._solved = None
        self.SetRansacParameters()

    # ---- upstream's parameters ----
    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        self.mRansacProb = float(probability)
        self.mRansacMinInliers = int(minInliers)
        N = self.N
        if self.mRansacMinInliers == N:
            n_it = 1
        else:
            # float epsilon = (float)minInliers / N; the rest in double (std::pow(float, int) is double)
            eps = float(np.float32(self.mRansacMinInliers) / np.float32(N)) if N else math.inf
            rest = 1.0 - eps * eps * eps
            # minInliers > N: upstream takes the logarithm of a negative number and iterate() gives up
            # at once (N < mRansacMinInliers); the cap stands
            n_it = maxIterations if rest <= 0.0 else _ceil_ratio(math.log(1.0 - self.mRansacProb), rest, maxIterations)
        self.mRansacMaxIts = max(1, min(n_it, int(maxIterations)))
        self.mnIterations = 0
        self._solved = None

    # ---- the device call ----
    def _problem(self, triples):
        t = np.ascontiguousarray(triples, np.int32).reshape(-1, 3)
        if t.shape[0] < self.mRansacMaxIts:
            raise ValueError(f"{t.shape[0]} triples for mRansacMaxIts = {self.mRansacMaxIts}")
        return np.ascontiguousarray(t[:self.mRansacMaxIts])

    def _runs(self) -> bool:   # iterate() returns before the loop otherwise
        return self.N >= max(3, self.mRansacMinInliers)

    def solve(self, triples):
        """All mRansacMaxIts hypotheses in one call; triples: at least mRansacMaxIts rows."""
        Sim3Solver.solve_batch([self], [triples])
        return self

    @staticmethod
    def solve_batch(solvers, triples_list):
        """Several candidates in one device call (up to 64); returns how many converge."""
        if len(solvers) != len(triples_list):
            raise ValueError("one triple array per solver")
        live = [(s, s._problem(t)) for s, t in zip(solvers, triples_list) if s._runs()]
        for s in solvers:
            s._solved = None
        if not live:
            return 0
        ctx = next((s.ctx for s, _ in live if s.ctx is not None), None)
        if ctx is None:   # made at the first call, not in the constructor: the state machine needs no device
            ctx = live[0][0].ctx = Context()
        B = len(live)
        probs, ress = (Sim3ProblemC * B)(), (Sim3ResultC * B)()
        outs = []
        for b, (s, t) in enumerate(live):
            H = t.shape[0]
            n_inl = np.zeros(H, np.int32)
            hyp = np.zeros((H, HYP_FLOATS), np.float32)
            inl = np.zeros(s.N, np.uint8)
            probs[b] = Sim3ProblemC((ctypes.c_float * 4)(*s.cam1), (ctypes.c_float * 4)(*s.cam2), s.N, ptr(s.X1),
                                    ptr(s.X2), ptr(s.max_err1), ptr(s.max_err2), int(s.fix_scale),
                                    s.mRansacMinInliers, H, ptr(t))
            ress[b].n_inliers, ress[b].hyp, ress[b].inliers = ptr(n_inl), ptr(hyp), ptr(inl)
            outs.append((t, n_inl, hyp, inl))
        rc = check(lib().orbhip_sim3_solve_batch(ctx.handle, probs, B, ress), "orbhip_sim3_solve_batch")
        for b, (s, _) in enumerate(live):
            t, n_inl, hyp, inl = outs[b]
            s._solved = dict(triples=t, n_inliers=n_inl, hyp=hyp, inliers=inl.astype(bool),
                             sel=np.array(ress[b].sel, np.float32), converged=int(ress[b].converged),
                             best=int(ress[b].best))
        return rc

    @staticmethod
    def T12_of(hyp13) -> np.ndarray:
        """mT12i = [s R | t] as float32 (s R elementwise, as the kernel forms it)."""
        h = np.asarray(hyp13, np.float32)
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = h[0] * h[1:10].reshape(3, 3)
        T[:3, 3] = h[10:13]
        return T

    # ---- upstream's iterate over the stored results ----
    def iterate(self, nIterations: int):
        """-> (T12, bNoMore, vbInliers, nInliers, bConverge), upstream's outputs for this chunk."""
        vbInliers = np.zeros(self.n1, bool)
        if self.N < self.mRansacMinInliers:
            return np.eye(4, dtype=np.float32), True, vbInliers, 0, False
        if self._solved is None:
            raise RuntimeError("Sim3Solver.iterate: call solve(triples) first")
        r = self._solved
        n_cur = 0
        while self.mnIterations < self.mRansacMaxIts and n_cur < nIterations:
            h = self.mnIterations
            n_cur += 1
            self.mnIterations += 1
            n_h = int(r["n_inliers"][h])
            if n_h >= self.mnBestInliers:
                self.mnBestInliers = n_h
                self.mBestT12 = self.T12_of(r["hyp"][h])
                if n_h > self.mRansacMinInliers:
                    # the first hypothesis above the minimum in the walk is the call's `converged`
                    assert h == r["converged"], (h, r["converged"])
                    vbInliers[self.indices1[r["inliers"]]] = True
                    return self.mBestT12.copy(), False, vbInliers, n_h, True
        return self.mBestT12.copy(), self.mnIterations >= self.mRansacMaxIts, vbInliers, 0, False

    def find(self):
        """upstream's find(): iterate(mRansacMaxIts)."""
        return self.iterate(self.mRansacMaxIts)


def _ceil_ratio(log_num: float, rest: float, cap: int) -> int:
    """ceil(log(1 - p) / log(rest)) as an int; rest == 1 (epsilon^3 below the double's resolution)
    divides by zero upstream, where the cap then stands."""
    den = math.log(rest)
    if den == 0.0:
        return cap
    v = math.ceil(log_num / den)
    return int(min(max(v, -2 ** 31), 2 ** 31 - 1))
