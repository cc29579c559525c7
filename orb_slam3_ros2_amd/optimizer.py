"""Optimizer mirror (U:src/Optimizer.cc) over liborbhip.so.

``Optimizer.LocalBundleAdjustment(problem)`` runs the g2o problem LocalBundleAdjustment
builds (VertexSE3Expmap poses, marginalised VertexSBAPointXYZ points, EdgeSE3ProjectXYZ
mono edges with Huber sqrt(5.991), BlockSolver_6_3 + Levenberg, optimize(10)) on the GPU
and returns the optimised poses/points and the per-edge chi2 / depth flags that the
reference uses to erase outlier observations (chi2 > 5.991 or depth <= 0).
``Optimizer.BundleAdjustment`` is the same solver with the GBA defaults.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import (BAProblemC, BAResultC, BAStereoProblemC, Context, EssentialGraphProblemC, EssentialGraphResultC,
                   PoseProblemC, PoseResultC, PoseStereoProblemC, Sim3OptProblemC, Sim3OptResultC, check, lib, ptr)

TH_HUBER_MONO = float(np.sqrt(np.float32(5.991)))
TH_HUBER_STEREO = float(np.sqrt(np.float32(7.815)))


@dataclass
class BAProblem:
    pose_q: np.ndarray          # [P,4] float32 (x,y,z,w), Tcw rotation
    pose_t: np.ndarray          # [P,3] float32
    pose_fixed: np.ndarray      # [P] uint8
    points: np.ndarray          # [M,3] float32 world
    edge_pose: np.ndarray       # [E] int32
    edge_point: np.ndarray      # [E] int32
    edge_uv: np.ndarray         # [E,2] float32
    edge_octave: np.ndarray     # [E] int32
    inv_sigma2: np.ndarray      # [L] float32
    fx: float
    fy: float
    cx: float
    cy: float
    huber_delta: float = TH_HUBER_MONO
    iterations: int = 10
    early_stop: int = 0

    def normalized(self) -> "BAProblem":
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
        return BAProblem(c(self.pose_q, np.float32), c(self.pose_t, np.float32), c(self.pose_fixed, np.uint8),
                         c(self.points, np.float32), c(self.edge_pose, np.int32), c(self.edge_point, np.int32),
                         c(self.edge_uv, np.float32), c(self.edge_octave, np.int32), c(self.inv_sigma2, np.float32),
                         float(self.fx), float(self.fy), float(self.cx), float(self.cy), float(self.huber_delta),
                         int(self.iterations), int(self.early_stop))

    def to_c(self) -> BAProblemC:
        return BAProblemC(self.pose_q.shape[0], self.points.shape[0], self.edge_pose.shape[0], ptr(self.pose_q),
                          ptr(self.pose_t), ptr(self.pose_fixed), ptr(self.points), ptr(self.edge_pose),
                          ptr(self.edge_point), ptr(self.edge_uv), ptr(self.edge_octave), ptr(self.inv_sigma2),
                          self.inv_sigma2.shape[0], self.fx, self.fy, self.cx, self.cy, self.huber_delta,
                          self.iterations, self.early_stop)


@dataclass
class StereoBAProblem(BAProblem):
    """A BAProblem of a rectified-stereo system: an observation with edge_ur >= 0 (the keyframe's
    mvuRight; 0.0 counts) is an EdgeStereoSE3ProjectXYZ with observation (u, v, ur) and the Huber
    delta huber_delta_stereo; the others stay monocular edges."""
    edge_ur: np.ndarray = None          # [E] float32 (< 0: a monocular edge)
    bf: float = 0.0                     # mbf
    huber_delta_stereo: float = TH_HUBER_STEREO

    def normalized(self) -> "StereoBAProblem":
        b = BAProblem.normalized(self)
        E = b.edge_pose.shape[0]
        ur = np.full(E, -1.0, np.float32) if self.edge_ur is None else \
            np.ascontiguousarray(self.edge_ur, dtype=np.float32).reshape(-1)
        if ur.shape[0] != E:
            raise ValueError("StereoBAProblem: edge_ur needs one entry per edge")
        return StereoBAProblem(**b.__dict__, edge_ur=ur, bf=float(self.bf),
                               huber_delta_stereo=float(self.huber_delta_stereo))

    def to_c(self) -> BAStereoProblemC:
        return BAStereoProblemC(BAProblem.to_c(self), ptr(self.edge_ur), self.bf, self.huber_delta_stereo)

    def mono(self) -> BAProblem:
        """The same problem without its right coordinates."""
        return BAProblem(**{k: v for k, v in self.__dict__.items()
                            if k not in ("edge_ur", "bf", "huber_delta_stereo")})

    def edge_thresholds(self) -> np.ndarray:
        """The chi2 at which upstream erases each observation: 7.815 stereo, 5.991 monocular."""
        ur = np.asarray(self.edge_ur, np.float32).reshape(-1)
        return np.where(ur >= 0, 7.815, 5.991)


@dataclass
class BAResult:
    pose_q: np.ndarray
    pose_t: np.ndarray
    points: np.ndarray
    edge_chi2: np.ndarray
    edge_depth_ok: np.ndarray
    initial_chi2: float
    final_chi2: float
    iterations_done: int
    lm_trials: int

    def outlier_edges(self, th=5.991) -> np.ndarray:
        """Edges LocalBundleAdjustment erases: chi2 > th || !isDepthPositive(). th: one threshold
        (5.991, monocular edges) or one per edge (StereoBAProblem.edge_thresholds(): 7.815 where
        edge_ur >= 0)."""
        return np.nonzero((self.edge_chi2 > np.asarray(th)) | (self.edge_depth_ok == 0))[0]


@dataclass
class PoseProblem:
    """The g2o problem Optimizer::PoseOptimization(Frame*) builds for one Frame: the initial Tcw
    and, per matched MapPoint, its world position and the undistorted keypoint. A rectified-stereo
    Frame also gives u_right (mvuRight; an entry >= 0 makes that observation a stereo edge, < 0
    leaves it monocular) and bf (mbf); without them the problem is the monocular one."""
    pose_q: np.ndarray          # [4] float32 (x,y,z,w), pFrame->GetPose() rotation
    pose_t: np.ndarray          # [3] float32
    points: np.ndarray          # [N,3] float32 MapPoint::GetWorldPos
    uv: np.ndarray              # [N,2] float32 mvKeysUn[i].pt
    octave: np.ndarray          # [N] int32 mvKeysUn[i].octave
    inv_sigma2: np.ndarray      # [L] float32 mvInvLevelSigma2
    fx: float
    fy: float
    cx: float
    cy: float
    u_right: np.ndarray | None = None   # [N] float32 mvuRight (None: a monocular Frame)
    bf: float = 0.0                     # mbf

    def normalized(self) -> "PoseProblem":
        c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)  # noqa: E731
        p = PoseProblem(c(self.pose_q, np.float32).reshape(4), c(self.pose_t, np.float32).reshape(3),
                        c(self.points, np.float32).reshape(-1, 3), c(self.uv, np.float32).reshape(-1, 2),
                        c(self.octave, np.int32).reshape(-1), c(self.inv_sigma2, np.float32),
                        float(self.fx), float(self.fy), float(self.cx), float(self.cy))
        if self.u_right is not None:
            p.u_right, p.bf = c(self.u_right, np.float32).reshape(-1), float(self.bf)
            if p.u_right.shape[0] != p.points.shape[0]:
                raise ValueError("PoseProblem: u_right needs one entry per correspondence")
        return p

    def to_c(self) -> PoseProblemC:
        return PoseProblemC(self.points.shape[0], ptr(self.pose_q), ptr(self.pose_t), ptr(self.points), ptr(self.uv),
                            ptr(self.octave), ptr(self.inv_sigma2), self.inv_sigma2.shape[0], self.fx, self.fy,
                            self.cx, self.cy)

    def to_c_stereo(self) -> PoseStereoProblemC:
        """The stereo entry's view of a normalized problem that carries u_right."""
        return PoseStereoProblemC(self.points.shape[0], ptr(self.pose_q), ptr(self.pose_t), ptr(self.points),
                                  ptr(self.uv), ptr(self.octave), ptr(self.inv_sigma2), self.inv_sigma2.shape[0],
                                  self.fx, self.fy, self.cx, self.cy, ptr(self.u_right), self.bf)


@dataclass
class PoseResult:
    pose_q: np.ndarray          # optimised Tcw
    pose_t: np.ndarray
    outlier: np.ndarray         # [N] uint8: mvbOutlier
    n_inliers: int              # PoseOptimization return value
    lm_trials: int


@dataclass
class Sim3Problem:
    """What Optimizer::OptimizeSim3's filter loop leaves of (pKF1, pKF2, vpMatches1, g2oS12): per kept
    correspondence the two map points in their cameras' frames, the two observations (obs2 of a match
    without a keypoint in KF2 is upstream's normalised x / z, y / z) and the two information values;
    the cameras; S12 as Eigen's quaternion (x, y, z, w), t, s in float64."""
    X1c: np.ndarray             # [N,3] float32 R1w X1w + t1w
    X2c: np.ndarray             # [N,3] float32
    obs1: np.ndarray            # [N,2] float32
    obs2: np.ndarray            # [N,2] float32
    inv_sigma2_1: np.ndarray    # [N] float32
    inv_sigma2_2: np.ndarray    # [N] float32
    cam1: np.ndarray            # [4] float32 fx, fy, cx, cy
    cam2: np.ndarray            # [4] float32
    q: np.ndarray               # [4] float64 (x, y, z, w)
    t: np.ndarray               # [3] float64
    s: float
    th2: float = 10.0
    fix_scale: bool = False

    def normalized(self) -> "Sim3Problem":
        c = lambda a, dt, shape: np.ascontiguousarray(a, dtype=dt).reshape(shape)  # noqa: E731
        p = Sim3Problem(c(self.X1c, np.float32, (-1, 3)), c(self.X2c, np.float32, (-1, 3)),
                        c(self.obs1, np.float32, (-1, 2)), c(self.obs2, np.float32, (-1, 2)),
                        c(self.inv_sigma2_1, np.float32, -1), c(self.inv_sigma2_2, np.float32, -1),
                        c(self.cam1, np.float32, 4), c(self.cam2, np.float32, 4), c(self.q, np.float64, 4),
                        c(self.t, np.float64, 3), float(self.s), float(self.th2), bool(self.fix_scale))
        n = p.X1c.shape[0]
        if not all(a.shape[0] == n for a in (p.X2c, p.obs1, p.obs2, p.inv_sigma2_1, p.inv_sigma2_2)):
            raise ValueError("Sim3Problem: every per-correspondence array needs the same length")
        return p

    def to_c(self) -> Sim3OptProblemC:
        f4, d4, d3 = ctypes.c_float * 4, ctypes.c_double * 4, ctypes.c_double * 3
        return Sim3OptProblemC(self.X1c.shape[0], ptr(self.X1c), ptr(self.X2c), ptr(self.obs1), ptr(self.obs2),
                               ptr(self.inv_sigma2_1), ptr(self.inv_sigma2_2), f4(*self.cam1), f4(*self.cam2),
                               d4(*self.q), d3(*self.t), self.s, self.th2, int(self.fix_scale))


@dataclass
class Sim3Result:
    q: np.ndarray               # [4] float64: the optimised g2oS12 (the input where n_in = 0 by the < 10 rule)
    t: np.ndarray               # [3] float64
    s: float
    n_in: int                   # OptimizeSim3's return value
    n_bad: int                  # pairs removed after the first round
    lm_trials: int
    keep: np.ndarray            # [N] uint8: 0 where upstream sets vpMatches1[idx] = NULL


@dataclass
class EssentialGraphProblem:
    """The graph Optimizer::OptimizeEssentialGraph builds from the Map, as arrays: VertexSim3Expmap
    estimates as g2o::Sim3 rows (Eigen's quaternion x, y, z, w, then t, then s; never renormalised) in
    the caller's order (recommended: keyframe id), the fixed flags, EdgeSim3 (i, j, Sji) edges with
    vertex(0) = i and vertex(1) = j, and the map points with their reference vertex."""
    S: np.ndarray               # [V,8] float64
    fixed: np.ndarray           # [V] uint8
    edge_ij: np.ndarray         # [E,2] int32
    edge_S: np.ndarray          # [E,8] float64: the measurement Sji
    fix_scale: bool = False
    iterations: int = 20
    lambda_init: float = 1e-16
    points: np.ndarray | None = None      # [M,3] float32
    point_ref: np.ndarray | None = None   # [M] int32

    def normalized(self) -> "EssentialGraphProblem":
        c = lambda a, dt, shape: np.ascontiguousarray(a, dtype=dt).reshape(shape)  # noqa: E731
        pts = c(self.points if self.points is not None else np.zeros((0, 3)), np.float32, (-1, 3))
        ref = c(self.point_ref if self.point_ref is not None else np.zeros(0), np.int32, -1)
        p = EssentialGraphProblem(c(self.S, np.float64, (-1, 8)), c(self.fixed, np.uint8, -1),
                                  c(self.edge_ij, np.int32, (-1, 2)), c(self.edge_S, np.float64, (-1, 8)),
                                  bool(self.fix_scale), int(self.iterations), float(self.lambda_init), pts, ref)
        if p.S.shape[0] != p.fixed.shape[0] or p.edge_ij.shape[0] != p.edge_S.shape[0] or \
                pts.shape[0] != ref.shape[0]:
            raise ValueError("EssentialGraphProblem: S / fixed, edge_ij / edge_S and points / point_ref need "
                             "the same lengths")
        return p

    def to_c(self) -> EssentialGraphProblemC:
        return EssentialGraphProblemC(self.S.shape[0], ptr(self.S), ptr(self.fixed), self.edge_ij.shape[0],
                                      ptr(self.edge_ij), ptr(self.edge_S), int(self.fix_scale), self.iterations,
                                      self.lambda_init, self.points.shape[0], ptr(self.points), ptr(self.point_ref))


@dataclass
class EssentialGraphResult:
    S: np.ndarray               # [V,8] float64: the corrected Siw (fixed vertices bit for bit the input)
    points: np.ndarray          # [M,3] float32: the corrected map points
    chi2_initial: float
    chi2_final: float
    iterations_run: int
    lm_trials: int
    lm_rejected: int
    solver: int                 # 0 the persistent tiled solver, 1 the blocked one, 2 blocked after a timeout


@dataclass
class BABatch:
    """A batch of problems in C-ABI form (Optimizer.prepare_batch); run_batch solves it in place."""
    problems: list
    outs: list
    cprobs: object
    cres: object


class Optimizer:
    def __init__(self, device: int = -1, ctx: Context | None = None):
        self.ctx = ctx or Context(device)

    def solve(self, prob: BAProblem, stop_flag: ctypes.c_int | None = None) -> BAResult:
        p = prob.normalized()
        P, M, E = p.pose_q.shape[0], p.points.shape[0], p.edge_pose.shape[0]
        # (every output word is written by the solve: no zero fill)
        out = BAResult(np.empty((P, 4), np.float32), np.empty((P, 3), np.float32), np.empty((M, 3), np.float32),
                       np.empty(E, np.float32), np.empty(E, np.uint8), 0.0, 0.0, 0, 0)
        rc = BAResultC(ptr(out.pose_q), ptr(out.pose_t), ptr(out.points), ptr(out.edge_chi2),
                       ptr(out.edge_depth_ok), 0.0, 0.0, 0, 0)
        pc = p.to_c()
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve(self.ctx.handle, ctypes.byref(pc), ctypes.byref(rc), sf), "orbhip_ba_solve")
        out.initial_chi2, out.final_chi2 = rc.initial_chi2, rc.final_chi2
        out.iterations_done, out.lm_trials = rc.iterations_done, rc.lm_trials
        return out

    def solve_stereo(self, prob: StereoBAProblem, stop_flag: ctypes.c_int | None = None) -> BAResult:
        """orbhip_ba_solve_stereo: one problem with EdgeStereoSE3ProjectXYZ edges where edge_ur >= 0."""
        p = prob.normalized()
        outs, cres = self._results_for([p])
        pc = p.to_c()
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_stereo(self.ctx.handle, ctypes.byref(pc), cres, sf), "orbhip_ba_solve_stereo")
        return self._fill(outs, cres)[0]

    def solve_stereo_batch(self, probs, stop_flag: ctypes.c_int | None = None):
        """orbhip_ba_solve_stereo_batch: B independent StereoBAProblems in one batched solve."""
        ps = [p.normalized() for p in probs]
        outs, cres = self._results_for(ps)
        cprobs = (BAStereoProblemC * len(ps))(*[p.to_c() for p in ps])
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_stereo_batch(self.ctx.handle, cprobs, len(ps), cres, sf),
              "orbhip_ba_solve_stereo_batch")
        return self._fill(outs, cres)

    def prepare_single(self, prob: BAProblem) -> "BABatch":
        """The C-ABI view of one problem (orbhip_ba_problem / orbhip_ba_result over the problem's
        own arrays and fresh outputs), as LocalMapping's C++ adapter holds it:
        run_single is the orbhip_ba_solve call alone, without solve()'s per-call marshalling."""
        p = prob.normalized()
        outs, cres = self._results_for([p])
        return BABatch([p], outs, p.to_c(), cres)

    def run_single(self, single: "BABatch", stop_flag: ctypes.c_int | None = None) -> BAResult:
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve(self.ctx.handle, ctypes.byref(single.cprobs), single.cres, sf), "orbhip_ba_solve")
        return self._fill(single.outs, single.cres)[0]

    def solve_batch(self, probs, stop_flag: ctypes.c_int | None = None):
        """B independent problems in one batched solve (replicas); returns a list of BAResult."""
        return self.run_batch(self.prepare_batch(probs), stop_flag)

    def prepare_batch(self, probs) -> "BABatch":
        """The C-ABI view of a batch (orbhip_ba_problem / orbhip_ba_result arrays over the
        problems' own arrays and freshly allocated outputs), as a C++ host adapter holds it: the
        Python marshalling is done once here, run_batch is the orbhip_ba_solve_batch call alone."""
        ps = [p.normalized() for p in probs]
        outs, cres = self._results_for(ps)
        cprobs = (BAProblemC * len(ps))(*[p.to_c() for p in ps])
        return BABatch(ps, outs, cprobs, cres)

    def run_batch(self, batch: "BABatch", stop_flag: ctypes.c_int | None = None):
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_batch(self.ctx.handle, batch.cprobs, len(batch.problems), batch.cres, sf),
              "orbhip_ba_solve_batch")
        return self._fill(batch.outs, batch.cres)

    # ---- sharded BundleAdjustment ----
    def _results_for(self, ps):
        outs, cres = [], (BAResultC * len(ps))()
        for i, p in enumerate(ps):
            P, M, E = p.pose_q.shape[0], p.points.shape[0], p.edge_pose.shape[0]
            o = BAResult(np.zeros((P, 4), np.float32), np.zeros((P, 3), np.float32), np.zeros((M, 3), np.float32),
                         np.zeros(E, np.float32), np.zeros(E, np.uint8), 0.0, 0.0, 0, 0)
            outs.append(o)
            cres[i] = BAResultC(ptr(o.pose_q), ptr(o.pose_t), ptr(o.points), ptr(o.edge_chi2), ptr(o.edge_depth_ok),
                                0.0, 0.0, 0, 0)
        return outs, cres

    @staticmethod
    def _fill(outs, cres):
        for o, r in zip(outs, cres):
            o.initial_chi2, o.final_chi2, o.iterations_done, o.lm_trials = (r.initial_chi2, r.final_chi2,
                                                                              r.iterations_done, r.lm_trials)
        return outs

    def solve_shards_local(self, shards, stop_flag: ctypes.c_int | None = None):
        """All shards of one problem in this process, summed on the device (orbhip_ba_solve_shards_local)."""
        ps = [p.normalized() for p in shards]
        outs, cres = self._results_for(ps)
        cprobs = (BAProblemC * len(ps))(*[p.to_c() for p in ps])
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_shards_local(self.ctx.handle, cprobs, len(ps), cres, sf),
              "orbhip_ba_solve_shards_local")
        return self._fill(outs, cres)

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (ctypes.c_uint8 * 128)()
        check(lib().orbhip_comm_unique_id(buf), "orbhip_comm_unique_id")
        return bytes(buf)

    def comm_init(self, nranks: int, rank: int, unique_id: bytes):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib().orbhip_comm_init(self.ctx.handle, int(nranks), int(rank), buf), "orbhip_comm_init")

    def solve_sharded(self, shard: BAProblem, stop_flag: ctypes.c_int | None = None) -> BAResult:
        """This rank's shard of a problem solved jointly over RCCL (after comm_init)."""
        p = shard.normalized()
        outs, cres = self._results_for([p])
        pc = p.to_c()
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_sharded(self.ctx.handle, ctypes.byref(pc), cres, sf), "orbhip_ba_solve_sharded")
        return self._fill(outs, cres)[0]

    def solve_sharded_segments(self, shards, stop_flag: ctypes.c_int | None = None):
        """This rank's consecutive shards (segments rank*len .. of nranks*len, sharding.shard_problem_nd)
        solved jointly over RCCL (after comm_init): summed on the device, then all-reduced."""
        ps = [p.normalized() for p in shards]
        outs, cres = self._results_for(ps)
        cprobs = (BAProblemC * len(ps))(*[p.to_c() for p in ps])
        sf = ctypes.addressof(stop_flag) if stop_flag is not None else None
        check(lib().orbhip_ba_solve_sharded_segments(self.ctx.handle, cprobs, len(ps), cres, sf),
              "orbhip_ba_solve_sharded_segments")
        return self._fill(outs, cres)

    def stats(self) -> dict:
        """orbhip_ba_stats: persistent-Cholesky launches on this device (all contexts), those that
        first waited for another stream's solve, the hand-off timeouts this context saw and the
        solves it re-ran on the non-persistent solvers."""
        out = (ctypes.c_int64 * 4)()
        check(lib().orbhip_ba_stats(self.ctx.handle, out), "orbhip_ba_stats")
        return dict(dag_launches=out[0], dag_handoffs=out[1], dag_timeouts=out[2], dag_reruns=out[3])

    def LocalBundleAdjustment(self, prob: BAProblem, stop_flag=None) -> BAResult:
        """A BAProblem or a StereoBAProblem (thHuberMono sqrt(5.991), thHuberStereo sqrt(7.815))."""
        if isinstance(prob, StereoBAProblem):
            return self.solve_stereo(prob, stop_flag)
        return self.solve(prob, stop_flag)

    def BundleAdjustment(self, prob: BAProblem, nIterations: int = 20, bRobust: bool = True,
                         stop_flag=None) -> BAResult:
        """A BAProblem or a StereoBAProblem (thHuber2D sqrt(5.99), thHuber3D sqrt(7.815))."""
        kw = {**prob.__dict__, "iterations": nIterations, "huber_delta": float(np.sqrt(5.99)) if bRobust else 0.0}
        if isinstance(prob, StereoBAProblem):
            kw["huber_delta_stereo"] = float(np.sqrt(7.815)) if bRobust else 0.0
            return self.solve_stereo(StereoBAProblem(**kw), stop_flag)
        return self.solve(BAProblem(**kw), stop_flag)

    # ---- motion-only BA ----
    def PoseOptimization(self, prob: PoseProblem) -> PoseResult:
        """U:src/Optimizer.cc::Optimizer::PoseOptimization(Frame*) for one frame."""
        return self.PoseOptimization_batch([prob])[0]

    def PoseOptimization_batch(self, probs) -> list:
        """Several frames in one launch (one wavefront per frame). When any problem carries u_right
        the batch takes the stereo entry, and every problem of it must carry one (all -1 for a
        monocular frame)."""
        ps = [p.normalized() for p in probs]
        outl = [np.zeros(p.points.shape[0], np.uint8) for p in ps]
        cres = (PoseResultC * len(ps))()
        for i, o in enumerate(outl):
            cres[i].outlier = ptr(o)
        if any(p.u_right is not None for p in ps):
            if any(p.u_right is None for p in ps):
                raise ValueError("PoseOptimization_batch: a stereo batch needs u_right in every problem "
                                 "(all -1 for a monocular frame)")
            cprobs = (PoseStereoProblemC * len(ps))(*[p.to_c_stereo() for p in ps])
            check(lib().orbhip_pose_optimization_stereo_batch(self.ctx.handle, cprobs, len(ps), cres),
                  "orbhip_pose_optimization_stereo_batch")
        else:
            cprobs = (PoseProblemC * len(ps))(*[p.to_c() for p in ps])
            check(lib().orbhip_pose_optimization_batch(self.ctx.handle, cprobs, len(ps), cres),
                  "orbhip_pose_optimization_batch")
        return [PoseResult(np.array(r.pose_q[:], np.float32), np.array(r.pose_t[:], np.float32), o, r.n_inliers,
                           r.lm_trials) for r, o in zip(cres, outl)]

    # ---- LoopClosing's Sim3 refinement ----
    def OptimizeSim3(self, prob: Sim3Problem) -> Sim3Result:
        """U:src/Optimizer.cc::Optimizer::OptimizeSim3 for one candidate (orbhip_optimize_sim3)."""
        p = prob.normalized()
        keep = np.zeros(p.X1c.shape[0], np.uint8)
        pc, r = p.to_c(), Sim3OptResultC()
        r.keep = ptr(keep)
        check(lib().orbhip_optimize_sim3(self.ctx.handle, ctypes.byref(pc), ctypes.byref(r)), "orbhip_optimize_sim3")
        return Sim3Result(np.array(r.q[:]), np.array(r.t[:]), r.s, r.n_in, r.n_bad, r.lm_trials, keep)

    def OptimizeSim3_batch(self, probs) -> list:
        """The candidates of one DetectCommonRegionsFromBoW round in one launch (one wavefront group
        per candidate; at most 64)."""
        ps = [p.normalized() for p in probs]
        if not ps:
            return []
        keeps = [np.zeros(p.X1c.shape[0], np.uint8) for p in ps]
        cres = (Sim3OptResultC * len(ps))()
        for i, k in enumerate(keeps):
            cres[i].keep = ptr(k)
        cprobs = (Sim3OptProblemC * len(ps))(*[p.to_c() for p in ps])
        check(lib().orbhip_optimize_sim3_batch(self.ctx.handle, cprobs, len(ps), cres), "orbhip_optimize_sim3_batch")
        return [Sim3Result(np.array(r.q[:]), np.array(r.t[:]), r.s, r.n_in, r.n_bad, r.lm_trials, k)
                for r, k in zip(cres, keeps)]

    # ---- CorrectLoop's / MergeLocal's pose graph ----
    def OptimizeEssentialGraph(self, prob: EssentialGraphProblem) -> EssentialGraphResult:
        """U:src/Optimizer.cc::Optimizer::OptimizeEssentialGraph and the map-point correction that
        follows it (orbhip_optimize_essential_graph)."""
        p = prob.normalized()
        S = np.zeros_like(p.S)
        pts = np.zeros_like(p.points)
        pc, r = p.to_c(), EssentialGraphResultC()
        r.S, r.points = ptr(S), ptr(pts)
        check(lib().orbhip_optimize_essential_graph(self.ctx.handle, ctypes.byref(pc), ctypes.byref(r)),
              "orbhip_optimize_essential_graph")
        return EssentialGraphResult(S, pts, r.chi2_initial, r.chi2_final, r.iterations_run, r.lm_trials,
                                    r.lm_rejected, r.solver)
