// vanishing_points.h -- the vanishing-point step of the reference's line front end (feature_tracker/src/line_feature_tracker.cpp:86-91:
// getVPHypVia2Lines, getSphereGrids, getBestVpsHyp, lines2Vps) in the reference's own terms, above uvs_vp_estimate(): key-line endpoints in,
// tmp_vps and local_vp_ids out, and the vp slots (12..14) of the 15-vector line messages filled as :379-385 does.  Header-only; the arithmetic
// is on the GPU (csrc/uvs_vanishing_points.hip).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "eigen_lite.h"

namespace uvs {

// what the step reads of a cv::line_descriptor::KeyLine: getStartPoint() / getEndPoint(), pixels of the undistorted image
struct KeyLineEnds { double sx, sy, ex, ey; };

class VanishingPoints {
public:
    // throws std::runtime_error without a GPU (no CPU path)
    explicit VanishingPoints(int device = 0, int max_lines = UVS_VP_MAX_LINES) {
        const int rc = uvs_vp_create(device, 1, max_lines, &vp_);
        if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_vp_create: ") + uvs_status_string(rc));
    }
    ~VanishingPoints() { uvs_vp_destroy(vp_); }
    VanishingPoints(const VanishingPoints&) = delete;
    VanishingPoints& operator=(const VanishingPoints&) = delete;

    // One frame (:86-91).  thAngle in radians (the reference: 1 degree); `seed` keys the sample generator (the reference seeds rand() with the
    // clock).  tmp_vps: three unit vectors; local_vp_ids: 0..2 per line, 3 for "none".  Returns UVS_OK or the error of uvs_vp_estimate (its
    // text in last_error); `last` holds the frame's uvs_vp_result.  A frame with fewer than two lines (which the reference skips) or without
    // a hypothesis leaves every id 3.
    int estimate(const std::vector<KeyLineEnds>& lines, const uvs_vp_camera& camera, double thAngle, uint64_t seed,
                 std::vector<Eigen::Vector3d>& tmp_vps, std::vector<int>& local_vp_ids) {
        const size_t n = lines.size();
        seg_.resize(4 * n); tag_.assign(n + 1, 3); lvp_.assign(3 * n + 3, 0.0);
        for (size_t l = 0; l < n; ++l) { seg_[4 * l] = lines[l].sx; seg_[4 * l + 1] = lines[l].sy; seg_[4 * l + 2] = lines[l].ex; seg_[4 * l + 3] = lines[l].ey; }
        uvs_vp_frame f;
        f.n_lines = (int32_t)n; f.reserved = 0; f.segments = seg_.data(); f.seed = seed;
        const int rc = uvs_vp_estimate(vp_, 1, &f, &camera, thAngle, tag_.data(), lvp_.data(), &last);
        if (rc != UVS_OK) { last_error = uvs_vp_last_error(vp_); return rc; }
        tmp_vps.assign(3, Eigen::Vector3d());
        for (int k = 0; k < 3; ++k) tmp_vps[k] = Eigen::Vector3d(last.vps[k][0], last.vps[k][1], last.vps[k][2]);
        local_vp_ids.assign(tag_.begin(), tag_.begin() + n);
        return UVS_OK;
    }

    // the vp of line l of the last estimate(): tmp_vps[id] / tmp_vps[id](2), or zero for id 3 (:379-385)
    Eigen::Vector3d lineVp(size_t l) const { return Eigen::Vector3d(lvp_[3 * l], lvp_[3 * l + 1], lvp_[3 * l + 2]); }

    // writes lineVp(l) into slots 12..14 of the l-th 15-vector line message (feature_manager.h:32-53)
    template <class Msg>
    void fillMessages(std::vector<Msg>& messages) const {
        for (size_t l = 0; l < messages.size(); ++l)
            for (int c = 0; c < 3; ++c) messages[l](12 + c) = lvp_[3 * l + c];
    }

    uvs_vp_result last{};
    std::string last_error;

private:
    uvs_vp_estimator* vp_ = nullptr;
    std::vector<double> seg_, lvp_;
    std::vector<int32_t> tag_;
};

}  // namespace uvs
