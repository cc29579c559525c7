"""orb_slam3_ros2_amd — MI355X-native ORB front-end + bundle-adjustment back-end.

Host-side mirror of the reference's hot-path interfaces over the C-ABI of
``liborbhip.so`` (include/orbhip.h):

  ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)      U:src/ORBextractor.cc
      __call__(image, mask, vLappingArea) -> (monoIndex, keypoints, descriptors)
  ORBmatcher.DescriptorDistance(a, b)                                       U:src/ORBmatcher.cc
  ORBmatcher(nnratio, checkOri).match_bf(...)                               (a12 rule)
  Optimizer.LocalBundleAdjustment(problem)                                  U:src/Optimizer.cc
  Optimizer.PoseOptimization(frame_problem)                                 U:src/Optimizer.cc
  ORBVocabulary(vocab).transform(desc)  (DBoW2 TemplatedVocabulary)         U:src/Frame.cc::ComputeBoW
  ORBmatcher.SearchByBoW(...)                                               U:src/ORBmatcher.cc
  ORBmatcher.SearchForInitialization(...)                                   U:src/ORBmatcher.cc
  ORBmatcher.SearchByProjectionLastFrame / SearchLocalPoints(...)           U:src/ORBmatcher.cc
  ORBmatcher.SearchForTriangulation(kf1, neighbours, ...)                   U:src/ORBmatcher.cc
  ORBmatcher.Fuse(kfs, points, ...)                                         U:src/ORBmatcher.cc
  ORBmatcher.FuseSim3 / SearchByProjectionSim3(...)   (LoopClosing)         U:src/ORBmatcher.cc
  Sim3Solver(...).solve(triples) / iterate(n) / solve_batch   (LoopClosing)  U:src/Sim3Solver.cc
  TwoViewReconstruction(K).Reconstruct(keys1, keys2, matches, sets)   (Tracking)  U:src/TwoViewReconstruction.cc
  Optimizer.OptimizeSim3(Sim3Problem) / OptimizeSim3_batch   (LoopClosing)   U:src/Optimizer.cc
  Optimizer.OptimizeEssentialGraph(EssentialGraphProblem)    (CorrectLoop)   U:src/Optimizer.cc
  KeyFrameDatabase(max_kf).DetectRelocalizationCandidates / DetectNBestCandidates
                                                                            U:src/KeyFrameDatabase.cc
  stereo_frame(ext, left, right, bf, b) -> StereoFrame   Frame's stereo ctor: both ExtractORB
                                                    calls + ComputeStereoMatches       U:src/Frame.cc
  FrameStream(w, h, frames_in_flight).push(frame)   Frame ctor -> ExtractORB + match to the last
                                                    frame, pipelined on the device

The HIP library is the only compute path: importing this package on a box without the
built extension, or calling it without a GPU, raises — there is no CPU fallback.
"""
from __future__ import annotations

from ._lib import OrbHipError, lib, library_path  # noqa: F401
from .extractor import KeyPoint, ORBextractor  # noqa: F401
from .matcher import ORBmatcher  # noqa: F401
from .optimizer import BAProblem, BAResult, Optimizer, PoseProblem, PoseResult, StereoBAProblem  # noqa: F401
from .optimizer import Sim3Problem, Sim3Result  # noqa: F401
from .optimizer import EssentialGraphProblem, EssentialGraphResult  # noqa: F401
from .bow import ORBVocabulary  # noqa: F401
from .kfdb import KeyFrameDatabase  # noqa: F401
from .frontend import FrameStream  # noqa: F401
from .camera import PinholeCamera  # noqa: F401
from .stereo import StereoFrame, stereo_frame  # noqa: F401
from .sim3solver import Sim3Solver, draw_triples  # noqa: F401
from .two_view import TwoViewReconstruction, draw_sets  # noqa: F401

__all__ = ["Sim3Solver", "draw_triples", "TwoViewReconstruction", "draw_sets", "StereoFrame", "stereo_frame", "ORBextractor", "KeyPoint", "ORBmatcher", "Optimizer", "BAProblem", "StereoBAProblem", "BAResult", "PoseProblem", "PoseResult", "Sim3Problem", "Sim3Result", "EssentialGraphProblem", "EssentialGraphResult", "ORBVocabulary", "KeyFrameDatabase", "FrameStream", "PinholeCamera",
           "OrbHipError",
           "lib", "library_path"]
