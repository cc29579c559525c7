// orbhip.hpp — C++ host mirror of the reference interfaces over the C-ABI of orbhip.h.
//
// Same names, argument meaning and error behaviour as the ORB_SLAM3 classes this path replaces
// (upstream ORB_SLAM3 v1.0, the gjcliff fork's submodule; cited U:file::Symbol because the
// submodule is empty in the reference tree):
//   U:include/ORBextractor.h  class ORBextractor   -> orbhip::ORBextractor
//   U:include/ORBmatcher.h    ORBmatcher::DescriptorDistance, TH_LOW / TH_HIGH / HISTO_LENGTH
//   U:include/Optimizer.h     Optimizer::LocalBundleAdjustment / BundleAdjustment (problem form)
// The reference types (cv::Mat, cv::KeyPoint, KeyFrame, MapPoint) stay on the adapter side
// (INTEGRATION.md). Here images are (pointer, w, h, stride) and keypoints are orbhip::KeyPoint
// with cv::KeyPoint's fields. Header-only: link liborbhip.so.
#ifndef ORBHIP_HPP
#define ORBHIP_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "orbhip.h"

namespace orbhip {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what + ": status " + std::to_string(code)), code_(code) {}
    int code() const { return code_; }

private:
    int code_;
};

inline void check(int rc, const char* what) {
    if (rc < 0) throw Error(rc, what);
}

// cv::KeyPoint's fields as ORBextractor fills them (class_id is always -1 there).
struct KeyPoint {
    float x, y, size, angle, response;
    int octave;
    int class_id = -1;
};

// U:include/ORBextractor.h::ORBextractor
class ORBextractor {
public:
    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
        : nfeatures_(nfeatures), scaleFactor_(scaleFactor), nlevels_(nlevels) {
        orbhip_orb_params p{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST};
        check(orbhip_create(&ctx_, device, &p), "orbhip_create");
        // the ctor's tables (U:src/ORBextractor.cc): mvScaleFactor from the library (float,
        // accumulated through the double scaleFactor), sigma2 = s*s, inverses in float
        mvScaleFactor_.resize(nlevels);
        check(orbhip_level_info(ctx_, 640, 480, nullptr, nullptr, nullptr, mvScaleFactor_.data()), "orbhip_level_info");
        for (int l = 0; l < nlevels; l++) {
            mvLevelSigma2_.push_back(mvScaleFactor_[l] * mvScaleFactor_[l]);
            mvInvScaleFactor_.push_back(1.0f / mvScaleFactor_[l]);
            mvInvLevelSigma2_.push_back(1.0f / mvLevelSigma2_[l]);
        }
    }
    ~ORBextractor() { if (ctx_) orbhip_destroy(ctx_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // operator()(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray descriptors,
    //            vector<int>& vLappingArea) -> monoIndex; -1 on an empty image. The mask is
    //            ignored by the reference as well. descriptors: N rows of 32 bytes.
    int operator()(const uint8_t* image, int w, int h, int stride, std::vector<KeyPoint>& keypoints,
                   std::vector<uint8_t>& descriptors, const std::vector<int>& vLappingArea) {
        keypoints.clear();
        descriptors.clear();
        if (!image || w <= 0 || h <= 0) return -1;
        const int cap = orbhip_max_keypoints(ctx_, w, h);
        check(cap, "orbhip_max_keypoints");
        kp_.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0, mono = 0;
        const int lap0 = vLappingArea.size() > 0 ? vLappingArea[0] : 0;
        const int lap1 = vLappingArea.size() > 1 ? vLappingArea[1] : 1000;
        const int rc = orbhip_extract(ctx_, image, w, h, stride, lap0, lap1, kp_.data(), descriptors.data(), cap, &n, &mono);
        if (rc == ORBHIP_ERR_EMPTY) return -1;
        check(rc, "orbhip_extract");
        keypoints.resize(n);
        for (int i = 0; i < n; i++)
            keypoints[i] = KeyPoint{kp_[i].x, kp_[i].y, kp_[i].size, kp_[i].angle, kp_[i].response, kp_[i].octave};
        descriptors.resize((size_t)n * 32);
        return mono;
    }

    int inline GetLevels() const { return nlevels_; }
    float inline GetScaleFactor() const { return scaleFactor_; }
    std::vector<float> inline GetScaleFactors() const { return mvScaleFactor_; }
    std::vector<float> inline GetInverseScaleFactors() const { return mvInvScaleFactor_; }
    std::vector<float> inline GetScaleSigmaSquares() const { return mvLevelSigma2_; }
    std::vector<float> inline GetInverseScaleSigmaSquares() const { return mvInvLevelSigma2_; }
    orbhip_ctx* context() const { return ctx_; }

private:
    orbhip_ctx* ctx_ = nullptr;
    int nfeatures_;
    float scaleFactor_;
    int nlevels_;
    std::vector<float> mvScaleFactor_, mvInvScaleFactor_, mvLevelSigma2_, mvInvLevelSigma2_;
    std::vector<orbhip_kp> kp_;
};

// U:src/Frame.cc, Frame(imLeft, imRight, ...): what the stereo constructor computes up to
// ComputeStereoMatches (both ExtractORB calls with vLappingArea {0, 0}, then mvuRight / mvDepth,
// -1 where a left keypoint has no stereo match).
struct StereoFrame {
    std::vector<KeyPoint> mvKeys, mvKeysRight;
    std::vector<uint8_t> mDescriptors, mDescriptorsRight;   // N rows of 32 bytes
    std::vector<float> mvuRight, mvDepth;
    std::vector<int32_t> status;                            // orbhip.h: 1 accepted, 2..9 the rejecting step
    int n_stereo = 0;
};

// mbf, mb as Frame holds them; center_patch: ORB_SLAM2's centre-subtracted patches. Returns false
// on an empty image. Both sides use the extractor's parameters (the reference builds
// mpORBextractorLeft / Right from the same settings).
inline bool ExtractStereo(ORBextractor& ext, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                          float mbf, float mb, StereoFrame& out, bool center_patch = false) {
    out = StereoFrame();
    if (!left || !right || w <= 0 || h <= 0) return false;
    const int cap = orbhip_max_keypoints(ext.context(), w, h);
    check(cap, "orbhip_max_keypoints");
    std::vector<orbhip_kp> kl(cap), kr(cap);
    out.mDescriptors.resize((size_t)cap * 32);
    out.mDescriptorsRight.resize((size_t)cap * 32);
    out.mvuRight.resize(cap);
    out.mvDepth.resize(cap);
    out.status.resize(cap);
    const orbhip_stereo_params prm{mbf, mb, center_patch ? 1 : 0};
    int nl = 0, nr = 0;
    check(orbhip_extract_stereo(ext.context(), left, right, w, h, stride, &prm, kl.data(), out.mDescriptors.data(), &nl,
                                kr.data(), out.mDescriptorsRight.data(), &nr, cap, out.mvuRight.data(),
                                out.mvDepth.data(), out.status.data(), &out.n_stereo),
          "orbhip_extract_stereo");
    for (int i = 0; i < nl; i++)
        out.mvKeys.push_back(KeyPoint{kl[i].x, kl[i].y, kl[i].size, kl[i].angle, kl[i].response, kl[i].octave});
    for (int i = 0; i < nr; i++)
        out.mvKeysRight.push_back(KeyPoint{kr[i].x, kr[i].y, kr[i].size, kr[i].angle, kr[i].response, kr[i].octave});
    out.mDescriptors.resize((size_t)nl * 32);
    out.mDescriptorsRight.resize((size_t)nr * 32);
    out.mvuRight.resize(nl);
    out.mvDepth.resize(nl);
    out.status.resize(nl);
    return true;
}

// U:include/ORBmatcher.h — the constants and the brute-force acceptance rule (a11/a12).
class ORBmatcher {
public:
    static const int TH_LOW = 50;
    static const int TH_HIGH = 100;
    static const int HISTO_LENGTH = 30;

    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orbhip_descriptor_distance(a, b); }

    // best/second over the whole train set; match[i] = train index or -1. Returns #matches.
    int MatchBruteForce(orbhip_ctx* ctx, const std::vector<uint8_t>& q, const std::vector<float>& qAngle,
                        const std::vector<uint8_t>& t, const std::vector<float>& tAngle, std::vector<int>& match,
                        int thLow = TH_LOW) const {
        const int nq = (int)(q.size() / 32), nt = (int)(t.size() / 32);
        match.assign(nq, -1);
        std::vector<int32_t> best(nq), second(nq);
        const int rc = orbhip_match_bf(ctx, q.data(), qAngle.data(), nq, t.data(), tAngle.data(), nt, thLow, mfNNratio,
                                       mbCheckOrientation ? 1 : 0, match.data(), best.data(), second.data());
        check(rc, "orbhip_match_bf");
        return rc;
    }

    // U:src/ORBmatcher.cc::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize):
    // keypoints/descriptors of both frames, F2's image bounds, vbPrevMatched as (x, y) pairs
    // (updated in place). Returns nmatches.
    int SearchForInitialization(orbhip_ctx* ctx, const std::vector<orbhip_kp>& kps1, const std::vector<uint8_t>& desc1,
                                const std::vector<orbhip_kp>& kps2, const std::vector<uint8_t>& desc2,
                                const float bounds2[4], std::vector<float>& vbPrevMatched,
                                std::vector<int>& vnMatches12, int windowSize = 10) const {
        vnMatches12.assign(kps1.size(), -1);
        const orbhip_init_frame f1{(int32_t)kps1.size(), kps1.data(), desc1.data(), 0.f, 1.f, 0.f, 1.f};
        const orbhip_init_frame f2{(int32_t)kps2.size(), kps2.data(), desc2.data(), bounds2[0], bounds2[1],
                                   bounds2[2], bounds2[3]};
        const int rc = orbhip_search_for_initialization(ctx, &f1, &f2, vbPrevMatched.data(), windowSize, mfNNratio,
                                                        mbCheckOrientation ? 1 : 0, vnMatches12.data());
        check(rc, "orbhip_search_for_initialization");
        return rc;
    }

    // U:src/ORBmatcher.cc::SearchByProjection(CurrentFrame, LastFrame, th, bMono = false) on a
    // rectified-stereo Frame (orbhip_stereo_view: the frame, mvuRight, mbf, mb). last: the LastFrame
    // entries with a non-outlier MapPoint; Tlw = LastFrame.GetPose(). vnMatches[q] = CurrentFrame
    // keypoint or -1; *direction (optional) = 1 forward, -1 backward, 0 neither. Returns nmatches.
    int SearchByProjectionStereo(orbhip_ctx* ctx, const orbhip_stereo_view& CurrentFrame, const orbhip_proj_last& last,
                                 const float Tlw_q[4], const float Tlw_t[3], float th, std::vector<int>& vnMatches,
                                 int* direction = nullptr) const {
        vnMatches.assign((size_t)std::max(last.n, 0), -1);
        int32_t dir = 0;
        const int rc = orbhip_search_by_projection_last_stereo(ctx, &CurrentFrame, &last, Tlw_q, Tlw_t, th,
                                                               mbCheckOrientation ? 1 : 0, vnMatches.data(), &dir);
        check(rc, "orbhip_search_by_projection_last_stereo");
        if (direction) *direction = dir;
        return rc;
    }

    // Tracking::SearchLocalPoints on a rectified-stereo Frame: Frame::isInFrustum (mbTrackInView,
    // mnTrackScaleLevel, mTrackProjXR) + SearchByProjection(F, vpMapPoints, th, bFarPoints,
    // thFarPoints) with the right-coordinate gate. mTrackProjXR is written where mbTrackInView.
    int SearchLocalPointsStereo(orbhip_ctx* ctx, const orbhip_stereo_view& F, const orbhip_local_points& mps, float th,
                                bool bFarPoints, float thFarPoints, std::vector<uint8_t>& mbTrackInView,
                                std::vector<int>& mnTrackScaleLevel, std::vector<float>& mTrackProjXR,
                                std::vector<int>& vnMatches, float viewingCosLimit = 0.5f) const {
        const size_t n = (size_t)std::max(mps.n, 0);
        mbTrackInView.assign(n, 0);
        mnTrackScaleLevel.assign(n, -1);
        mTrackProjXR.resize(n);
        vnMatches.assign(n, -1);
        const int rc = orbhip_search_local_points_stereo(ctx, &F, &mps, viewingCosLimit, th, mfNNratio,
                                                         bFarPoints ? 1 : 0, thFarPoints, mbTrackInView.data(),
                                                         mnTrackScaleLevel.data(), mTrackProjXR.data(), vnMatches.data());
        check(rc, "orbhip_search_local_points_stereo");
        return rc;
    }

    // U:src/ORBmatcher.cc::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, false, false) of pKF1
    // against every neighbour in one call (LocalMapping::CreateNewMapPoints).
    // vMatches12[b][i] = neighbour b's feature matched to pKF1's feature i, or -1 (vMatchedPairs of
    // pair b = the (i, vMatches12[b][i]) with a match, in i order). Returns the matches per neighbour.
    std::vector<int> SearchForTriangulation(orbhip_ctx* ctx, const orbhip_tri_keyframe& kf1,
                                            const std::vector<orbhip_tri_keyframe>& neighbours,
                                            const std::vector<float>& mvScaleFactors,
                                            const std::vector<float>& mvLevelSigma2,
                                            std::vector<std::vector<int>>& vMatches12) const {
        const int B = (int)neighbours.size(), n1 = kf1.n;
        std::vector<int32_t> flat((size_t)B * (size_t)std::max(n1, 0), -1), nm(B, 0);
        const int rc = orbhip_search_for_triangulation(ctx, &kf1, neighbours.data(), B, mvScaleFactors.data(),
                                                       mvLevelSigma2.data(),
                                                       (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()),
                                                       mbCheckOrientation ? 1 : 0, flat.data(), nm.data());
        check(rc, "orbhip_search_for_triangulation");
        vMatches12.assign(B, std::vector<int>());
        for (int b = 0; b < B; b++) vMatches12[b].assign(flat.begin() + (size_t)b * n1, flat.begin() + (size_t)(b + 1) * n1);
        return std::vector<int>(nm.begin(), nm.end());
    }

    // One new MapPoint of LocalMapping::CreateNewMapPoints: pKF1's feature idx1 and neighbour nbr's
    // feature idx2 triangulated to x3D.
    struct NewMapPoint {
        int nbr, idx1, idx2;
        float x3D[3];
    };

    // the mandatory outputs of an orbhip_new_points (the optional diagnostics stay NULL)
    struct NewPointsBuffers {
        std::vector<int32_t> nmatches, nnew, first, nbr, idx1, idx2;
        std::vector<uint8_t> gated;
        std::vector<float> x3d;
        orbhip_new_points out{};
        NewPointsBuffers(int B, int n1)
            : nmatches(std::max(B, 1)), nnew(std::max(B, 1)), first(std::max(n1, 1)), nbr(std::max(n1, 1)),
              idx1(std::max(n1, 1)), idx2(std::max(n1, 1)), gated(std::max(B, 1)), x3d(3 * (size_t)std::max(n1, 1)) {
            out.nmatches = nmatches.data(); out.gated = gated.data(); out.first = first.data();
            out.nnew = nnew.data(); out.new_nbr = nbr.data(); out.new_idx1 = idx1.data();
            out.new_idx2 = idx2.data(); out.new_x3d = x3d.data();
        }
        std::vector<NewMapPoint> list(int n) const {
            std::vector<NewMapPoint> v((size_t)n);
            for (int k = 0; k < n; k++) v[k] = {nbr[k], idx1[k], idx2[k], {x3d[3 * k], x3d[3 * k + 1], x3d[3 * k + 2]}};
            return v;
        }
    };

    // U:src/LocalMapping.cc::CreateNewMapPoints from the search to the accepted points, in one call
    // (INTEGRATION.md §3d): SearchForTriangulation of pKF1 against every neighbour with this matcher's
    // mbCheckOrientation, then the triangulation and its checks. vMedianDepth: empty, or per neighbour
    // its ComputeSceneMedianDepth(2) (the baseline gate; vbGated, optional, receives who it stopped).
    // ratioFactor = 1.5f * mfScaleFactor; thFarPoints <= 0: off. Returns the new points in upstream's
    // creation order (ascending neighbour, then ascending idx1), one per feature of pKF1: that of the
    // first neighbour that accepts it.
    std::vector<NewMapPoint> CreateNewMapPoints(orbhip_ctx* ctx, const orbhip_tri_keyframe& kf1,
                                                const std::vector<orbhip_tri_keyframe>& neighbours,
                                                const std::vector<float>& vMedianDepth,
                                                const std::vector<float>& mvScaleFactors,
                                                const std::vector<float>& mvLevelSigma2, float ratioFactor,
                                                double cosParallaxMax = 0.9998, float thFarPoints = 0.f,
                                                std::vector<uint8_t>* vbGated = nullptr) const {
        const int B = (int)neighbours.size();
        if (!vMedianDepth.empty() && (int)vMedianDepth.size() != B) check(ORBHIP_ERR_ARG, "CreateNewMapPoints");
        NewPointsBuffers buf(B, kf1.n);
        const orbhip_tri_params prm{cosParallaxMax, ratioFactor, thFarPoints};
        const int n = orbhip_create_new_map_points(ctx, &kf1, neighbours.data(), B,
                                                   vMedianDepth.empty() ? nullptr : vMedianDepth.data(),
                                                   mvScaleFactors.data(), mvLevelSigma2.data(),
                                                   (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()),
                                                   mbCheckOrientation ? 1 : 0, &prm, &buf.out);
        check(n, "orbhip_create_new_map_points");
        if (vbGated) vbGated->assign(buf.gated.begin(), buf.gated.begin() + B);
        return buf.list(n);
    }

    // The same from given matches (vMatches12[b][i] = neighbour b's feature or -1): no search, no gate.
    std::vector<NewMapPoint> TriangulateMatches(orbhip_ctx* ctx, const orbhip_tri_keyframe& kf1,
                                                const std::vector<orbhip_tri_keyframe>& neighbours,
                                                const std::vector<std::vector<int>>& vMatches12,
                                                const std::vector<float>& mvScaleFactors,
                                                const std::vector<float>& mvLevelSigma2, float ratioFactor,
                                                double cosParallaxMax = 0.9998, float thFarPoints = 0.f) const {
        const int B = (int)neighbours.size(), n1 = std::max(kf1.n, 0);
        if ((int)vMatches12.size() != B) check(ORBHIP_ERR_ARG, "TriangulateMatches");
        std::vector<int32_t> flat((size_t)B * n1 + 1, -1);
        for (int b = 0; b < B; b++) {
            if ((int)vMatches12[b].size() != n1) check(ORBHIP_ERR_ARG, "TriangulateMatches");
            std::copy(vMatches12[b].begin(), vMatches12[b].end(), flat.begin() + (size_t)b * n1);
        }
        NewPointsBuffers buf(B, kf1.n);
        const orbhip_tri_params prm{cosParallaxMax, ratioFactor, thFarPoints};
        const int n = orbhip_triangulate_matches(ctx, &kf1, neighbours.data(), B, flat.data(), mvScaleFactors.data(),
                                                 mvLevelSigma2.data(),
                                                 (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()), &prm,
                                                 &buf.out);
        check(n, "orbhip_triangulate_matches");
        return buf.list(n);
    }

    // The three calls above for a rectified-stereo system (orbhip_tri_stereo_keyframe: the keyframe,
    // mvuRight, mvDepth, mbf, mb): no epipole exclusion for a pair with a stereo
    // feature, a neighbour gated when the baseline is below its mb (there is no vMedianDepth), the
    // stereo parallax with UnprojectStereo and the three-term reprojection test. vSource (optional,
    // B x n1 flat) receives upstream's bPointStereo per pair: 0 none, 1 triangulated, 2 / 3
    // unprojected from pKF1 / the neighbour.
    std::vector<int> SearchForTriangulation(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe& kf1,
                                            const std::vector<orbhip_tri_stereo_keyframe>& neighbours,
                                            const std::vector<float>& mvScaleFactors,
                                            const std::vector<float>& mvLevelSigma2,
                                            std::vector<std::vector<int>>& vMatches12) const {
        const int B = (int)neighbours.size(), n1 = kf1.kf.n;
        std::vector<int32_t> flat((size_t)B * (size_t)std::max(n1, 0), -1), nm(B, 0);
        const int rc = orbhip_search_for_triangulation_stereo(ctx, &kf1, neighbours.data(), B, mvScaleFactors.data(),
                                                              mvLevelSigma2.data(),
                                                              (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()),
                                                              mbCheckOrientation ? 1 : 0, flat.data(), nm.data());
        check(rc, "orbhip_search_for_triangulation_stereo");
        vMatches12.assign(B, std::vector<int>());
        for (int b = 0; b < B; b++) vMatches12[b].assign(flat.begin() + (size_t)b * n1, flat.begin() + (size_t)(b + 1) * n1);
        return std::vector<int>(nm.begin(), nm.end());
    }

    std::vector<NewMapPoint> CreateNewMapPoints(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe& kf1,
                                                const std::vector<orbhip_tri_stereo_keyframe>& neighbours,
                                                const std::vector<float>& mvScaleFactors,
                                                const std::vector<float>& mvLevelSigma2, float ratioFactor,
                                                double cosParallaxMax = 0.9998, float thFarPoints = 0.f,
                                                std::vector<uint8_t>* vbGated = nullptr,
                                                std::vector<uint8_t>* vSource = nullptr) const {
        const int B = (int)neighbours.size();
        NewPointsBuffers buf(B, kf1.kf.n);
        if (vSource) vSource->assign((size_t)B * (size_t)std::max(kf1.kf.n, 0) + 1, 0);
        const orbhip_tri_params prm{cosParallaxMax, ratioFactor, thFarPoints};
        const int n = orbhip_create_new_map_points_stereo(ctx, &kf1, neighbours.data(), B, mvScaleFactors.data(),
                                                          mvLevelSigma2.data(),
                                                          (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()),
                                                          mbCheckOrientation ? 1 : 0, &prm, &buf.out,
                                                          vSource ? vSource->data() : nullptr);
        check(n, "orbhip_create_new_map_points_stereo");
        if (vbGated) vbGated->assign(buf.gated.begin(), buf.gated.begin() + B);
        if (vSource) vSource->pop_back();
        return buf.list(n);
    }

    std::vector<NewMapPoint> TriangulateMatches(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe& kf1,
                                                const std::vector<orbhip_tri_stereo_keyframe>& neighbours,
                                                const std::vector<std::vector<int>>& vMatches12,
                                                const std::vector<float>& mvScaleFactors,
                                                const std::vector<float>& mvLevelSigma2, float ratioFactor,
                                                double cosParallaxMax = 0.9998, float thFarPoints = 0.f,
                                                std::vector<uint8_t>* vSource = nullptr) const {
        const int B = (int)neighbours.size(), n1 = std::max(kf1.kf.n, 0);
        if ((int)vMatches12.size() != B) check(ORBHIP_ERR_ARG, "TriangulateMatches");
        std::vector<int32_t> flat((size_t)B * n1 + 1, -1);
        for (int b = 0; b < B; b++) {
            if ((int)vMatches12[b].size() != n1) check(ORBHIP_ERR_ARG, "TriangulateMatches");
            std::copy(vMatches12[b].begin(), vMatches12[b].end(), flat.begin() + (size_t)b * n1);
        }
        NewPointsBuffers buf(B, kf1.kf.n);
        if (vSource) vSource->assign((size_t)B * n1 + 1, 0);
        const orbhip_tri_params prm{cosParallaxMax, ratioFactor, thFarPoints};
        const int n = orbhip_triangulate_matches_stereo(ctx, &kf1, neighbours.data(), B, flat.data(),
                                                        mvScaleFactors.data(), mvLevelSigma2.data(),
                                                        (int)std::min(mvScaleFactors.size(), mvLevelSigma2.size()), &prm,
                                                        &buf.out, vSource ? vSource->data() : nullptr);
        check(n, "orbhip_triangulate_matches_stereo");
        if (vSource) vSource->pop_back();
        return buf.list(n);
    }

    // U:src/ORBmatcher.cc::Fuse(pKF, vpMapPoints, th) of every keyframe against the same MapPoints in
    // one call (LocalMapping::SearchInNeighbors). vbPairSkip: empty, or B x n with
    // pMP->IsInKeyFrame(keyframe b). vBestIdx[b][m] = the keypoint of keyframe b MapPoint m fuses into,
    // or -1; the adapter applies Replace / AddObservation / AddMapPoint in upstream order. vBestDist /
    // vLevel (optional) receive the winning distance and nPredictedLevel. Returns the fused points per
    // keyframe.
    std::vector<int> Fuse(orbhip_ctx* ctx, const std::vector<orbhip_frame>& keyframes,
                          const orbhip_local_points& vpMapPoints, const std::vector<uint8_t>& vbPairSkip,
                          const std::vector<float>& mvInvLevelSigma2, float th,
                          std::vector<std::vector<int>>& vBestIdx, std::vector<std::vector<int>>* vBestDist = nullptr,
                          std::vector<std::vector<int>>* vLevel = nullptr) const {
        for (const orbhip_frame& f : keyframes)
            if ((size_t)std::max(f.n_levels, 0) > mvInvLevelSigma2.size()) throw Error(ORBHIP_ERR_ARG, "Fuse: mvInvLevelSigma2");
        return fuseRows((int)keyframes.size(), vpMapPoints, vbPairSkip, vBestIdx, vBestDist, vLevel, "orbhip_fuse",
                        [&](const uint8_t* skip, int32_t* idx, int32_t* dist, int32_t* lvl, int32_t* nf) {
                            return orbhip_fuse(ctx, keyframes.data(), (int)keyframes.size(), &vpMapPoints, skip,
                                               mvInvLevelSigma2.data(), th, idx, dist, lvl, nf);
                        });
    }

    // Fuse on rectified-stereo keyframes (orbhip_stereo_view: the keyframe, mvuRight, mbf, mb): a
    // candidate keypoint with mvuRight >= 0 is gated on (ex, ey, er) at 7.8, the others as above
    // (orbhip_fuse_stereo). Arguments and results as the monocular overload.
    std::vector<int> Fuse(orbhip_ctx* ctx, const std::vector<orbhip_stereo_view>& keyframes,
                          const orbhip_local_points& vpMapPoints, const std::vector<uint8_t>& vbPairSkip,
                          const std::vector<float>& mvInvLevelSigma2, float th,
                          std::vector<std::vector<int>>& vBestIdx, std::vector<std::vector<int>>* vBestDist = nullptr,
                          std::vector<std::vector<int>>* vLevel = nullptr) const {
        for (const orbhip_stereo_view& f : keyframes)
            if ((size_t)std::max(f.frame.n_levels, 0) > mvInvLevelSigma2.size())
                throw Error(ORBHIP_ERR_ARG, "Fuse: mvInvLevelSigma2");
        return fuseRows((int)keyframes.size(), vpMapPoints, vbPairSkip, vBestIdx, vBestDist, vLevel, "orbhip_fuse_stereo",
                        [&](const uint8_t* skip, int32_t* idx, int32_t* dist, int32_t* lvl, int32_t* nf) {
                            return orbhip_fuse_stereo(ctx, keyframes.data(), (int)keyframes.size(), &vpMapPoints, skip,
                                                      mvInvLevelSigma2.data(), th, idx, dist, lvl, nf);
                        });
    }

    // What the Fuse overloads share: the pair-skip check, the flat outputs, the call (call(pair_skip,
    // best_idx, best_dist, level, nfused) returns the entry point's status) and the rows per keyframe.
    template <class Call>
    static std::vector<int> fuseRows(int B, const orbhip_local_points& vpMapPoints, const std::vector<uint8_t>& vbPairSkip,
                                     std::vector<std::vector<int>>& vBestIdx, std::vector<std::vector<int>>* vBestDist,
                                     std::vector<std::vector<int>>* vLevel, const char* what, Call call) {
        const size_t n = (size_t)std::max(vpMapPoints.n, 0);
        if (!vbPairSkip.empty() && vbPairSkip.size() != (size_t)B * n) throw Error(ORBHIP_ERR_ARG, "Fuse: vbPairSkip");
        std::vector<int32_t> idx((size_t)B * n, -1), dist(vBestDist ? (size_t)B * n : 0), lvl(vLevel ? (size_t)B * n : 0);
        std::vector<int32_t> nf(B, 0);
        check(call(vbPairSkip.empty() ? nullptr : vbPairSkip.data(), idx.data(), vBestDist ? dist.data() : nullptr,
                   vLevel ? lvl.data() : nullptr, nf.data()), what);
        auto rows = [&](const std::vector<int32_t>& flat, std::vector<std::vector<int>>& out) {
            out.assign(B, std::vector<int>());
            for (int b = 0; b < B; b++) out[b].assign(flat.begin() + (size_t)b * n, flat.begin() + (size_t)(b + 1) * n);
        };
        rows(idx, vBestIdx);
        if (vBestDist) rows(dist, *vBestDist);
        if (vLevel) rows(lvl, *vLevel);
        return std::vector<int>(nf.begin(), nf.end());
    }

    // U:src/ORBmatcher.cc::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) of every keyframe against the
    // same MapPoints in one call (LoopClosing::SearchAndFuse). Each orbhip_frame
    // carries Tcw = (Scw.rotationMatrix(), Scw.translation() / Scw.scale()). vbPairSkip: empty, or
    // B x n with pKF_b->GetMapPoints().count(pMP). Outputs as Fuse; the adapter fills vpReplacePoint
    // from pKF->GetMapPoint(vBestIdx[b][m]) or calls AddObservation / AddMapPoint.
    std::vector<int> FuseSim3(orbhip_ctx* ctx, const std::vector<orbhip_frame>& keyframes,
                              const orbhip_local_points& vpPoints, const std::vector<uint8_t>& vbPairSkip, float th,
                              std::vector<std::vector<int>>& vBestIdx, std::vector<std::vector<int>>* vBestDist = nullptr,
                              std::vector<std::vector<int>>* vLevel = nullptr) const {
        const int B = (int)keyframes.size();
        const size_t n = (size_t)std::max(vpPoints.n, 0);
        if (!vbPairSkip.empty() && vbPairSkip.size() != (size_t)B * n) throw Error(ORBHIP_ERR_ARG, "FuseSim3: vbPairSkip");
        std::vector<int32_t> idx((size_t)B * n, -1), dist(vBestDist ? (size_t)B * n : 0), lvl(vLevel ? (size_t)B * n : 0);
        std::vector<int32_t> nf(B, 0);
        const int rc = orbhip_fuse_sim3(ctx, keyframes.data(), B, &vpPoints, vbPairSkip.empty() ? nullptr : vbPairSkip.data(),
                                        th, idx.data(), vBestDist ? dist.data() : nullptr, vLevel ? lvl.data() : nullptr,
                                        nf.data());
        check(rc, "orbhip_fuse_sim3");
        auto rows = [&](const std::vector<int32_t>& flat, std::vector<std::vector<int>>& out) {
            out.assign(B, std::vector<int>());
            for (int b = 0; b < B; b++) out[b].assign(flat.begin() + (size_t)b * n, flat.begin() + (size_t)(b + 1) * n);
        };
        rows(idx, vBestIdx);
        if (vBestDist) rows(dist, *vBestDist);
        if (vLevel) rows(lvl, *vLevel);
        return std::vector<int>(nf.begin(), nf.end());
    }

    // U:src/ORBmatcher.cc::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (and the
    // overload with vpPointsKFs / vpMatchedKF), the sequential greedy pass exactly. keyframe carries
    // Tcw = (R, t / s) and claimed[k] = vpMatched[k] != NULL; vpPoints.skip[m] = isBad() or the point
    // is in vpMatched already. vnMatch[m] = the keypoint point m claims, or -1 (the adapter sets
    // vpMatched[vnMatch[m]] = vpPoints[m]). Returns nmatches.
    int SearchByProjectionSim3(orbhip_ctx* ctx, const orbhip_frame& keyframe, const orbhip_local_points& vpPoints, int th,
                               float ratioHamming, std::vector<int>& vnMatch, std::vector<int>* vnDist = nullptr,
                               std::vector<int>* vnLevel = nullptr) const {
        const size_t n = (size_t)std::max(vpPoints.n, 0);
        std::vector<int32_t> m(n, -1), dist(vnDist ? n : 0), lvl(vnLevel ? n : 0);
        const int rc = orbhip_search_by_projection_sim3(ctx, &keyframe, &vpPoints, (float)th, ratioHamming, m.data(),
                                                        vnDist ? dist.data() : nullptr, vnLevel ? lvl.data() : nullptr);
        check(rc, "orbhip_search_by_projection_sim3");
        vnMatch.assign(m.begin(), m.end());
        if (vnDist) vnDist->assign(dist.begin(), dist.end());
        if (vnLevel) vnLevel->assign(lvl.begin(), lvl.end());
        return rc;
    }

    float mfNNratio;
    bool mbCheckOrientation;
};

// U:include/Sim3Solver.h — Horn's closed form on RANSAC triples; every hypothesis in one device call
// (orbhip_sim3_solve_batch), then upstream's iterate() over the stored results.
// The adapter fills the correspondences its constructor's filter leaves: X1 / X2 (the map points in
// the two cameras' frames), the truncated error bounds (MaxError), indices1 = mvnIndices1, n1 = mN1.
class Sim3Solver {
public:
    // mvnMaxError: upstream keeps 9.210 * sigma2 in a vector<size_t>
    static float MaxError(float sigma2) { return (float)(size_t)(9.210 * (double)sigma2); }

    // upstream's draw from a fresh mvAllIndices per iteration; RandomInt(lo, hi), both ends included
    template <class RandomInt>
    static std::vector<int32_t> DrawTriples(int N, int H, RandomInt&& randint) {
        std::vector<int32_t> out((size_t)H * 3), avail;
        for (int h = 0; h < H; h++) {
            avail.resize(N);
            for (int i = 0; i < N; i++) avail[i] = i;
            for (int k = 0; k < 3; k++) {
                const int r = randint(0, (int)avail.size() - 1);
                out[(size_t)3 * h + k] = avail[r];
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
        return out;
    }

    std::vector<float> X1, X2, vMaxError1, vMaxError2;   // N x 3, N x 3, N, N
    std::vector<int> vnIndices1;                         // N
    int mN1 = 0;
    float cam1[4] = {0, 0, 0, 0}, cam2[4] = {0, 0, 0, 0};   // fx, fy, cx, cy
    bool mbFixScale = false;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0;
    float mBestT12[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // row-major 4 x 4

    int N() const { return (int)vMaxError1.size(); }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        int nIterations = maxIterations;
        if (minInliers == N()) {
            nIterations = 1;
        } else if (N() > 0) {
            const float epsilon = (float)minInliers / N();
            const double rest = 1.0 - std::pow((double)epsilon, 3);
            if (rest > 0.0 && rest < 1.0) {
                const double v = std::ceil(std::log(1.0 - probability) / std::log(rest));
                nIterations = v < (double)maxIterations ? (int)v : maxIterations;
            }
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, maxIterations));
        mnIterations = 0;
        solved_ = false;
    }

    // every one of the mRansacMaxIts hypotheses in one call; vTriples: at least mRansacMaxIts x 3
    void solve(orbhip_ctx* ctx, const std::vector<int32_t>& vTriples) {
        solved_ = false;
        if (N() < std::max(3, mRansacMinInliers)) return;   // iterate() gives up at once
        if (vTriples.size() < (size_t)mRansacMaxIts * 3) throw Error(ORBHIP_ERR_ARG, "Sim3Solver: vTriples");
        orbhip_sim3_problem p{};
        std::memcpy(p.cam1, cam1, sizeof cam1);
        std::memcpy(p.cam2, cam2, sizeof cam2);
        p.n = N(); p.X1 = X1.data(); p.X2 = X2.data(); p.max_err1 = vMaxError1.data(); p.max_err2 = vMaxError2.data();
        p.fix_scale = mbFixScale; p.min_inliers = mRansacMinInliers; p.n_hyp = mRansacMaxIts; p.triples = vTriples.data();
        nInliers_.assign(mRansacMaxIts, 0);
        hyp_.assign((size_t)mRansacMaxIts * 13, 0.f);
        inliers_.assign(N(), 0);
        orbhip_sim3_result r{};
        r.n_inliers = nInliers_.data(); r.hyp = hyp_.data(); r.inliers = inliers_.data();
        check(orbhip_sim3_solve(ctx, &p, &r), "orbhip_sim3_solve");
        solved_ = true;
    }

    // upstream's iterate(): returns mBestT12 (row-major 4 x 4, [s R | t])
    const float* iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge) {
        static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        bNoMore = false;
        bConverge = false;
        vbInliers.assign(mN1, false);
        nInliers = 0;
        if (N() < mRansacMinInliers) { bNoMore = true; return kIdentity; }
        if (!solved_) throw Error(ORBHIP_ERR_ARG, "Sim3Solver::iterate before solve");
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            const int h = mnIterations;
            nCurrentIterations++;
            mnIterations++;
            if (nInliers_[h] >= mnBestInliers) {
                mnBestInliers = nInliers_[h];
                const float* y = &hyp_[(size_t)13 * h];
                for (int i = 0; i < 3; i++) {
                    for (int j = 0; j < 3; j++) mBestT12[4 * i + j] = y[0] * y[1 + 3 * i + j];
                    mBestT12[4 * i + 3] = y[10 + i];
                }
                if (nInliers_[h] > mRansacMinInliers) {   // h == the call's `converged`: its mask came back
                    nInliers = nInliers_[h];
                    for (int i = 0; i < N(); i++)
                        if (inliers_[i]) vbInliers[vnIndices1[i]] = true;
                    bConverge = true;
                    return mBestT12;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return mBestT12;
    }

private:
    std::vector<int32_t> nInliers_;
    std::vector<float> hyp_;
    std::vector<uint8_t> inliers_;
    bool solved_ = false;
};

// U:include/TwoViewReconstruction.h — the homography / fundamental-matrix RANSAC of monocular
// initialisation, the model choice and the motion recovery in one device call
// (orbhip_two_view_reconstruct). The adapter passes the undistorted keypoints of
// the two frames and vMatches12 as Tracking holds them, and the 8-sets from DrawSets.
class TwoViewReconstruction {
public:
    // K as (fx, fy, cx, cy); sigma and iterations as upstream's constructor takes them
    TwoViewReconstruction(const float K[4], float sigma = 1.0f, int iterations = 200)
        : mSigma(sigma), mMaxIterations(iterations) {
        std::memcpy(mK, K, sizeof mK);
    }

    // upstream's draw from a fresh vAvailableIndices per iteration; RandomInt(lo, hi), both ends
    // included (upstream calls DUtils::Random::SeedRandOnce(0) first). N = the number of matches
    template <class RandomInt>
    static std::vector<int32_t> DrawSets(int N, int H, RandomInt&& randint) {
        if (N < 8) throw Error(ORBHIP_ERR_ARG, "TwoViewReconstruction::DrawSets: N < 8");
        std::vector<int32_t> out((size_t)H * 8), avail;
        for (int h = 0; h < H; h++) {
            avail.resize(N);
            for (int i = 0; i < N; i++) avail[i] = i;
            for (int k = 0; k < 8; k++) {
                const int r = randint(0, (int)avail.size() - 1);
                out[(size_t)8 * h + k] = avail[r];
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
        return out;
    }

    // Reconstruct(vKeys1, vKeys2, vMatches12, T21, vP3D, vbTriangulated): T21 row-major 4 x 4, vP3D
    // n1 x 3; vSets: at least mMaxIterations x 8 indices into the matches in index order. The
    // diagnostics of the call stay in `last`.
    bool Reconstruct(orbhip_ctx* ctx, const std::vector<orbhip_kp>& vKeys1, const std::vector<orbhip_kp>& vKeys2,
                     const std::vector<int>& vMatches12, const std::vector<int32_t>& vSets, float T21[16],
                     std::vector<float>& vP3D, std::vector<bool>& vbTriangulated) {
        if (vMatches12.size() != vKeys1.size()) throw Error(ORBHIP_ERR_ARG, "TwoViewReconstruction: vMatches12");
        if (vSets.size() < (size_t)mMaxIterations * 8) throw Error(ORBHIP_ERR_ARG, "TwoViewReconstruction: vSets");
        const std::vector<int32_t> m(vMatches12.begin(), vMatches12.end());
        orbhip_two_view_problem p{};
        p.n1 = (int32_t)vKeys1.size(); p.n2 = (int32_t)vKeys2.size();
        p.kps1 = vKeys1.data(); p.kps2 = vKeys2.data(); p.matches12 = m.data();
        std::memcpy(p.K, mK, sizeof mK);
        p.sigma = mSigma; p.n_hyp = mMaxIterations; p.sets = vSets.data();
        vP3D.assign(vKeys1.size() * 3, 0.f);
        std::vector<uint8_t> tri(vKeys1.size(), 0);
        last = orbhip_two_view_result{};
        last.p3d = vP3D.data(); last.triangulated = tri.data();
        check(orbhip_two_view_reconstruct(ctx, &p, &last), "orbhip_two_view_reconstruct");
        last.p3d = nullptr; last.triangulated = nullptr;
        vbTriangulated.assign(tri.begin(), tri.end());
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) T21[4 * i + j] = last.R21[3 * i + j];
            T21[4 * i + 3] = last.t21[i];
            T21[12 + i] = 0.f;
        }
        T21[15] = 1.f;
        return last.success != 0;
    }

    float mK[4];
    float mSigma;
    int mMaxIterations;
    orbhip_two_view_result last{};
};

// U:include/KeyFrameDatabase.h — the device database; slots stand for KeyFrames.
class KeyFrameDatabase {
public:
    KeyFrameDatabase(orbhip_ctx* ctx, int maxKF) : maxKF_(maxKF) { check(orbhip_kfdb_create(ctx, maxKF, &db_), "orbhip_kfdb_create"); }
    ~KeyFrameDatabase() { if (db_) orbhip_kfdb_destroy(db_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
    void add(int kf, const std::vector<int32_t>& words, const std::vector<double>& values) {
        check(orbhip_kfdb_add(db_, kf, words.data(), values.data(), (int)words.size()), "orbhip_kfdb_add");
    }
    void erase(int kf) { check(orbhip_kfdb_erase(db_, kf), "orbhip_kfdb_erase"); }
    std::vector<int> DetectRelocalizationCandidates(const orbhip_kfdb_query& q) {
        std::vector<int32_t> out(maxKF_);
        const int n = orbhip_kfdb_detect_relocalization(db_, &q, out.data(), maxKF_);
        check(n, "orbhip_kfdb_detect_relocalization");
        return std::vector<int>(out.begin(), out.begin() + std::min(n, maxKF_));
    }
    void DetectNBestCandidates(const orbhip_kfdb_query& q, const std::vector<uint8_t>& connected, int n,
                               std::vector<int>& loopCand, std::vector<int>& mergeCand) {
        std::vector<int32_t> lo(n > 0 ? n : 1), me(n > 0 ? n : 1);
        int32_t nl = 0, nm = 0;
        check(orbhip_kfdb_detect_nbest(db_, &q, connected.empty() ? nullptr : connected.data(), n, lo.data(), &nl,
                                       me.data(), &nm), "orbhip_kfdb_detect_nbest");
        loopCand.assign(lo.begin(), lo.begin() + nl);
        mergeCand.assign(me.begin(), me.begin() + nm);
    }

private:
    orbhip_kfdb* db_ = nullptr;
    int maxKF_;
};

// U:include/Optimizer.h — the g2o problem of LocalBundleAdjustment in SoA form. The adapter
// fills it from the local KeyFrames / MapPoints and applies the result.
struct BAProblem {
    std::vector<float> pose_q, pose_t, points, edge_uv, inv_sigma2;
    std::vector<uint8_t> pose_fixed;
    std::vector<int32_t> edge_pose, edge_point, edge_octave;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    float huber_delta = std::sqrt(5.991f);
    int iterations = 10;
    int early_stop = 0;
};

struct BAResult {
    std::vector<float> pose_q, pose_t, points, edge_chi2;
    std::vector<uint8_t> edge_depth_ok;
    double initial_chi2 = 0, final_chi2 = 0;
    int iterations_done = 0, lm_trials = 0;
};

// A BAProblem of a rectified-stereo system: an observation with edge_ur[e] >= 0 (mvuRight; 0.0f counts)
// is an EdgeStereoSE3ProjectXYZ with the Huber delta huber_delta_stereo, the others monocular edges
struct StereoBAProblem : BAProblem {
    std::vector<float> edge_ur;          // one per edge (< 0: a monocular edge)
    float bf = 0.0f;                     // mbf
    float huber_delta_stereo = 2.7955321f;   // sqrt(7.815): thHuberStereo (LBA), thHuber3D (GBA)
};

// What OptimizeSim3's filter loop leaves of (pKF1, pKF2, vpMatches1): per kept correspondence the two
// map points in their cameras' frames, the two observations and the two information values
struct Sim3Problem {
    std::vector<float> X1c, X2c;                  // N x 3: R1w X1w + t1w, R2w X2w + t2w
    std::vector<float> obs1, obs2;                // N x 2 (obs2 of a match without a keypoint: upstream's x / z, y / z)
    std::vector<float> inv_sigma2_1, inv_sigma2_2;   // N
    float cam1[4] = {0, 0, 0, 0}, cam2[4] = {0, 0, 0, 0};   // fx, fy, cx, cy
};

// The graph OptimizeEssentialGraph builds from the Map: VertexSim3Expmap estimates (q xyzw, t, s per
// vertex, in keyframe-id order for a near-diagonal system), the fixed flags, EdgeSim3 (i, j, Sji)
// edges with vertex(0) = i, and the map points with the vertex of their reference keyframe
struct EssentialGraph {
    std::vector<double> S;            // V x 8, in and out
    std::vector<uint8_t> fixed;       // V
    std::vector<int32_t> edge_ij;     // E x 2
    std::vector<double> edge_S;       // E x 8: Sji
    std::vector<float> points;        // M x 3, in and out
    std::vector<int32_t> point_ref;   // M
};
struct EssentialGraphResult {
    double chi2_initial, chi2_final;
    int iterations_run, lm_trials, lm_rejected, solver;
};

class Optimizer {
public:
    // LocalBundleAdjustment's optimize(10) with Huber sqrt(5.991). The reference's bool*
    // pbStopFlag (LocalMapping::mbAbortBA -> g2o setForceStopFlag) is an int here, polled by
    // the solver between LM iterations and trials; NULL = never stop.
    static BAResult LocalBundleAdjustment(orbhip_ctx* ctx, const BAProblem& p, const volatile int* pbStopFlag = nullptr) {
        return solve(ctx, p, pbStopFlag);
    }
    // BundleAdjustment(vpKF, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust): robust -> sqrt(5.99)
    static BAResult BundleAdjustment(orbhip_ctx* ctx, BAProblem p, int nIterations = 5,
                                     const volatile int* pbStopFlag = nullptr, bool bRobust = true) {
        p.iterations = nIterations;
        p.huber_delta = bRobust ? std::sqrt(5.99f) : 0.0f;
        return solve(ctx, p, pbStopFlag);
    }

    // The same two with stereo edges (orbhip_ba_solve_stereo): edge_chi2 of a stereo edge is the
    // three-term chi2, which the caller erases at 7.815 (5.991 on the monocular edges)
    static BAResult LocalBundleAdjustment(orbhip_ctx* ctx, const StereoBAProblem& p,
                                          const volatile int* pbStopFlag = nullptr) {
        return solve(ctx, p, pbStopFlag, &p);
    }
    static BAResult BundleAdjustment(orbhip_ctx* ctx, StereoBAProblem p, int nIterations = 5,
                                     const volatile int* pbStopFlag = nullptr, bool bRobust = true) {
        p.iterations = nIterations;
        p.huber_delta = bRobust ? std::sqrt(5.99f) : 0.0f;
        p.huber_delta_stereo = bRobust ? std::sqrt(7.815f) : 0.0f;
        return solve(ctx, p, pbStopFlag, &p);
    }

    // PoseOptimization(Frame*) of a rectified-stereo Frame: observations with u_right >= 0 are
    // EdgeStereoSE3ProjectXYZOnlyPose edges, the others monocular. Tcw (q: x, y, z, w) is updated in
    // place (pFrame->SetPose), mvbOutlier gets one flag per correspondence. Returns
    // nInitialCorrespondences - nBad.
    static int PoseOptimizationStereo(orbhip_ctx* ctx, orbhip_pose_stereo_problem p, float Tcw_q[4], float Tcw_t[3],
                                      std::vector<uint8_t>& mvbOutlier) {
        p.pose_q = Tcw_q;
        p.pose_t = Tcw_t;
        mvbOutlier.assign((size_t)std::max(p.n, 0), 0);
        orbhip_pose_result r{};
        r.outlier = mvbOutlier.data();
        const int rc = orbhip_pose_optimization_stereo(ctx, &p, &r);
        check(rc, "orbhip_pose_optimization_stereo");
        for (int k = 0; k < 4; k++) Tcw_q[k] = r.pose_q[k];
        for (int k = 0; k < 3; k++) Tcw_t[k] = r.pose_t[k];
        return rc;
    }

    // OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, ...): the adapter's filter loop fills
    // the Sim3Problem; g2oS12 = (q: x, y, z, w; t; s) is updated in place unless
    // the call returns 0 by the "fewer than 10 left" rule, vbKeep gets 0 where upstream sets
    // vpMatches1[idx] = NULL. Returns nIn.
    static int OptimizeSim3(orbhip_ctx* ctx, const Sim3Problem& p, double q[4], double t[3], double& s, float th2,
                            bool bFixScale, std::vector<uint8_t>& vbKeep, int* pnBad = nullptr) {
        const size_t n = p.inv_sigma2_1.size();
        if (p.X1c.size() != 3 * n || p.X2c.size() != 3 * n || p.obs1.size() != 2 * n || p.obs2.size() != 2 * n ||
            p.inv_sigma2_2.size() != n)
            throw std::invalid_argument("Sim3Problem: every array needs one entry per correspondence");
        orbhip_sim3_opt_problem c{};
        c.n = (int32_t)n;
        c.X1c = p.X1c.data(); c.X2c = p.X2c.data(); c.obs1 = p.obs1.data(); c.obs2 = p.obs2.data();
        c.inv_sigma2_1 = p.inv_sigma2_1.data(); c.inv_sigma2_2 = p.inv_sigma2_2.data();
        std::memcpy(c.cam1, p.cam1, sizeof c.cam1);
        std::memcpy(c.cam2, p.cam2, sizeof c.cam2);
        for (int k = 0; k < 4; k++) c.q[k] = q[k];
        for (int k = 0; k < 3; k++) c.t[k] = t[k];
        c.s = s; c.th2 = th2; c.fix_scale = bFixScale;
        vbKeep.assign(n, 0);
        orbhip_sim3_opt_result r{};
        r.keep = vbKeep.data();
        const int rc = orbhip_optimize_sim3(ctx, &c, &r);
        check(rc, "orbhip_optimize_sim3");
        for (int k = 0; k < 4; k++) q[k] = r.q[k];
        for (int k = 0; k < 3; k++) t[k] = r.t[k];
        s = r.s;
        if (pnBad) *pnBad = r.n_bad;
        return rc;
    }

    // OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections,
    // bFixScale) and MergeLocal's overload: the adapter builds the graph from the Map (INTEGRATION.md
    // 3i) and decides which vertices are fixed. Returns the corrected Siw in g.S (n x 8: q xyzw, t,
    // s; the adapter sets Tiw = [R | t / s]) and the corrected map points in g.points.
    static EssentialGraphResult OptimizeEssentialGraph(orbhip_ctx* ctx, EssentialGraph& g, bool bFixScale,
                                                       int nIterations = 20, double lambdaInit = 1e-16) {
        const size_t nv = g.fixed.size(), ne = g.edge_ij.size() / 2, np = g.point_ref.size();
        if (g.S.size() != 8 * nv || g.edge_ij.size() != 2 * ne || g.edge_S.size() != 8 * ne || g.points.size() != 3 * np)
            throw std::invalid_argument("EssentialGraph: S / fixed, edge_ij / edge_S and points / point_ref need the same lengths");
        orbhip_essential_graph_problem c{};
        c.n_vertices = (int32_t)nv; c.S = g.S.data(); c.fixed = g.fixed.data();
        c.n_edges = (int32_t)ne; c.edge_ij = g.edge_ij.data(); c.edge_S = g.edge_S.data();
        c.fix_scale = bFixScale; c.iterations = nIterations; c.lambda_init = lambdaInit;
        c.n_points = (int32_t)np; c.points = g.points.data(); c.point_ref = g.point_ref.data();
        std::vector<double> S(8 * nv);
        std::vector<float> pts(3 * np);
        orbhip_essential_graph_result r{};
        r.S = S.data(); r.points = pts.data();
        check(orbhip_optimize_essential_graph(ctx, &c, &r), "orbhip_optimize_essential_graph");
        g.S.swap(S);
        g.points.swap(pts);
        return EssentialGraphResult{r.chi2_initial, r.chi2_final, r.iterations_run, r.lm_trials, r.lm_rejected, r.solver};
    }

private:
    static BAResult solve(orbhip_ctx* ctx, const BAProblem& p, const volatile int* stop,
                          const StereoBAProblem* stereo = nullptr) {
        const int P = (int)p.pose_fixed.size(), M = (int)(p.points.size() / 3), E = (int)p.edge_pose.size();
        orbhip_ba_problem c{P, M, E, p.pose_q.data(), p.pose_t.data(), p.pose_fixed.data(), p.points.data(),
                            p.edge_pose.data(), p.edge_point.data(), p.edge_uv.data(), p.edge_octave.data(),
                            p.inv_sigma2.data(), (int)p.inv_sigma2.size(), p.fx, p.fy, p.cx, p.cy, p.huber_delta,
                            p.iterations, p.early_stop};
        BAResult r;
        r.pose_q.resize(4 * (size_t)P); r.pose_t.resize(3 * (size_t)P); r.points.resize(3 * (size_t)M);
        r.edge_chi2.resize(E); r.edge_depth_ok.resize(E);
        orbhip_ba_result o{r.pose_q.data(), r.pose_t.data(), r.points.data(), r.edge_chi2.data(), r.edge_depth_ok.data(),
                           0, 0, 0, 0};
        if (stereo) {
            if (stereo->edge_ur.size() != (size_t)E) throw std::invalid_argument("StereoBAProblem: edge_ur needs one entry per edge");
            orbhip_ba_stereo_problem sc{c, stereo->edge_ur.data(), stereo->bf, stereo->huber_delta_stereo};
            check(orbhip_ba_solve_stereo(ctx, &sc, &o, stop), "orbhip_ba_solve_stereo");
        } else {
            check(orbhip_ba_solve(ctx, &c, &o, stop), "orbhip_ba_solve");
        }
        r.initial_chi2 = o.initial_chi2; r.final_chi2 = o.final_chi2;
        r.iterations_done = o.iterations_done; r.lm_trials = o.lm_trials;
        return r;
    }
};

// Camera front-end stream (orbhip_frontend_*): push device frames, read slots when needed.
class FrameStream {
public:
    FrameStream(int w, int h, int frames_in_flight = 8, int device = 0, orbhip_orb_params prm = {1000, 1.2f, 8, 20, 7},
                int th_low = 50, float nnratio = 0.9f, bool check_orientation = true) {
        check(orbhip_frontend_create(&fe_, device, &prm, w, h, frames_in_flight, th_low, nnratio,
                                     check_orientation ? 1 : 0),
              "orbhip_frontend_create");
    }
    ~FrameStream() {
        if (fe_) orbhip_frontend_destroy(fe_);
    }
    FrameStream(const FrameStream&) = delete;
    FrameStream& operator=(const FrameStream&) = delete;
    // returns the slot that will hold this frame's keypoints and its match to the previous frame
    int push(const uint8_t* d_gray, int stride, int lap0 = 0, int lap1 = 1000) {
        const int slot = orbhip_frontend_push(fe_, d_gray, stride, lap0, lap1);
        check(slot, "orbhip_frontend_push");
        return slot;
    }
    orbhip_frontend_slot view(int slot) const {
        orbhip_frontend_slot v{};
        check(orbhip_frontend_view(fe_, slot, &v), "orbhip_frontend_view");
        return v;
    }
    void wait(int slot, void* stream = nullptr) const { check(orbhip_frontend_wait(fe_, slot, stream), "orbhip_frontend_wait"); }

private:
    orbhip_frontend* fe_ = nullptr;
};

}  // namespace orbhip

#endif  // ORBHIP_HPP
