// feature_tracker.h -- the reference's point front end (feature_tracker/src/feature_tracker.cpp:54-147, 184-196, 240-288: readImage, addPoints,
// updateID, undistortedPoints) in the reference's own terms, above uvs_ft_track(): an image in, cur_pts / ids / track_cnt / cur_un_pts /
// pts_velocity out.  Header-only.  The optical flow, the inBorder cut and liftProjective of the tracked points are on the GPU
// (csrc/uvs_feature_track.hip); what is here is the bookkeeping around them.  Differences from the reference, all from the C ABI below:
// positions are FP64 (cv::Point2f there), new points are the caller's (goodFeaturesToTrack + setMask there), rejectWithF and CLAHE are not here,
// and n_id is a member, not a static, so that two trackers of one process number their points apart.
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "../csrc/uvs_camera_lift.h"

namespace uvs {

struct Point2d { double x = 0.0, y = 0.0; };

// utility.cpp:11-18 / feature_tracker.cpp's reduceVector: keeps v[i] where status[i]
template <class T>
inline void reduceVector(std::vector<T>& v, const std::vector<uint8_t>& status) {
    size_t j = 0;
    for (size_t i = 0; i < v.size(); ++i)
        if (status[i]) v[j++] = v[i];
    v.resize(j);
}

// The bookkeeping of readImage without the device: what happens to the vectors once the flow of a frame is known.  FeatureTracker below feeds
// it from uvs_ft_track; a test may feed it by hand.
class FeatureTrackerBook {
public:
    explicit FeatureTrackerBook(const uvs_kf_camera& camera) : camera_(camera), lift_(uvs_lift_camera(camera)) {}

    // :81-107 after the flow: forw_pts = next_xy, status[i] = (ft_status[i] == UVS_FT_TRACKED) (the device has applied inBorder), the six
    // reduceVector calls, track_cnt++.  next_norm: liftProjective of next_xy from the device.
    void applyFlow(double time, const std::vector<Point2d>& next_xy, const std::vector<int32_t>& ft_status, const std::vector<Point2d>& next_norm) {
        cur_time = time;
        forw_pts = next_xy; forw_norm_ = next_norm;
        std::vector<uint8_t> status(ft_status.size());
        for (size_t i = 0; i < status.size(); ++i) status[i] = ft_status[i] == UVS_FT_TRACKED;
        if (!cur_pts.empty()) {
            reduceVector(prev_pts, status); reduceVector(cur_pts, status); reduceVector(forw_pts, status); reduceVector(ids, status);
            reduceVector(cur_un_pts, status); reduceVector(track_cnt, status); reduceVector(forw_norm_, status);
        }
        for (auto& n : track_cnt) n++;
    }

    // :44-52
    void addPoints() {
        for (const auto& p : n_pts) { forw_pts.push_back(p); ids.push_back(-1); track_cnt.push_back(1); }
    }

    // :140-146
    void rotate() {
        prev_pts = cur_pts; prev_un_pts = cur_un_pts; cur_pts = forw_pts;
        undistortedPoints();
        prev_time = cur_time;
    }

    // :184-196
    bool updateID(unsigned int i) {
        if (i < ids.size()) {
            if (ids[i] == -1) ids[i] = n_id++;
            return true;
        }
        return false;
    }

    // :240-288.  The normalized coordinates of the tracked points are the device's; a point added in this frame is lifted here by the same
    // function (uvs_camera_lift.h).  std::map::insert keeps the first entry of a key, as the reference's does for the ids still -1.
    void undistortedPoints() {
        cur_un_pts.clear(); cur_un_pts_map.clear();
        for (size_t i = 0; i < cur_pts.size(); ++i) {
            Point2d b;
            if (i < forw_norm_.size()) b = forw_norm_[i];
            else uvs_lift_projective(lift_, cur_pts[i].x, cur_pts[i].y, b.x, b.y);
            cur_un_pts.push_back(b);
            cur_un_pts_map.insert(std::make_pair(ids[i], b));
        }
        pts_velocity.clear();
        if (!prev_un_pts_map.empty()) {
            const double dt = cur_time - prev_time;
            for (size_t i = 0; i < cur_un_pts.size(); ++i) {
                Point2d v;
                if (ids[i] != -1) {
                    const auto it = prev_un_pts_map.find(ids[i]);
                    if (it != prev_un_pts_map.end()) { v.x = (cur_un_pts[i].x - it->second.x) / dt; v.y = (cur_un_pts[i].y - it->second.y) / dt; }
                }
                pts_velocity.push_back(v);
            }
        } else {
            pts_velocity.assign(cur_pts.size(), Point2d());
        }
        prev_un_pts_map = cur_un_pts_map;
    }

    std::vector<Point2d> n_pts, prev_pts, cur_pts, forw_pts, prev_un_pts, cur_un_pts, pts_velocity;
    std::vector<int> ids, track_cnt;
    std::map<int, Point2d> cur_un_pts_map, prev_un_pts_map;
    double cur_time = 0.0, prev_time = 0.0;
    int n_id = 0;

protected:
    uvs_kf_camera camera_;
    UvsLiftCam lift_;
    std::vector<Point2d> forw_norm_;
};

class FeatureTracker : public FeatureTrackerBook {
public:
    // where goodFeaturesToTrack sits (:119-131): called with the tracker after the flow (forw_pts are the tracked points), fills n_pts
    using Detector = std::function<void(const FeatureTracker&, std::vector<Point2d>&)>;

    // throws std::runtime_error without a GPU (no CPU path)
    FeatureTracker(const uvs_kf_camera& camera, int device = 0, int max_width = 752, int max_height = 480, int levels = 4, int max_points = 1024)
        : FeatureTrackerBook(camera) {
        const int rc = uvs_ft_create(device, 1, max_width, max_height, levels, max_points, &ft_);
        if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_ft_create: ") + uvs_status_string(rc));
    }
    ~FeatureTracker() { uvs_ft_destroy(ft_); }
    FeatureTracker(const FeatureTracker&) = delete;
    FeatureTracker& operator=(const FeatureTracker&) = delete;

    // :54-147 with PUB_THIS_FRAME set.  image: [height][width] grey levels (after CLAHE, if the caller wants it).  Returns UVS_OK or the error
    // of uvs_ft_track (its text in last_error; the vectors are unchanged then).
    int readImage(const uint8_t* image, int width, int height, double time, const Detector& detect = nullptr) {
        const size_t n = cur_pts.size();
        xy_.resize(2 * n + 2); nxt_.resize(2 * n + 2); nrm_.resize(2 * n + 2); st_.resize(n + 1); it_.resize(n + 1);
        for (size_t i = 0; i < n; ++i) { xy_[2 * i] = cur_pts[i].x; xy_[2 * i + 1] = cur_pts[i].y; }
        uvs_ft_item item;
        item.image = image; item.stream = 0; item.width = width; item.height = height; item.n_points = (int32_t)n; item.points_xy = n ? xy_.data() : nullptr;
        int32_t n_tracked = 0;
        const int rc = uvs_ft_track(ft_, 1, &item, &camera_, nxt_.data(), st_.data(), it_.data(), nrm_.data(), &n_tracked);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        std::vector<Point2d> next(n), norm(n);
        for (size_t i = 0; i < n; ++i) { next[i].x = nxt_[2 * i]; next[i].y = nxt_[2 * i + 1]; norm[i].x = nrm_[2 * i]; norm[i].y = nrm_[2 * i + 1]; }
        applyFlow(time, next, std::vector<int32_t>(st_.begin(), st_.begin() + n), norm);
        n_pts.clear();
        if (detect) detect(*this, n_pts);
        addPoints();
        rotate();
        return UVS_OK;
    }

    std::string last_error;

private:
    uvs_ft_tracker* ft_ = nullptr;
    std::vector<double> xy_, nxt_, nrm_;
    std::vector<int32_t> st_, it_;
};

}  // namespace uvs
