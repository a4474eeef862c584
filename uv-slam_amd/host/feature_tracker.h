// feature_tracker.h -- the reference's point front end (feature_tracker/src/feature_tracker.cpp:9-196, 240-288: setMask, addPoints, readImage,
// rejectWithF, updateID, undistortedPoints) in the reference's own terms, above uvs_ft_track(), uvs_ft_reject() and uvs_ft_detect(): an image
// in, cur_pts / ids / track_cnt / cur_un_pts / pts_velocity out.  Header-only.  The optical flow, the inBorder cut, the fundamental-matrix
// RANSAC, the detection of new points and liftProjective are on the GPU (csrc/uvs_feature_track.hip, csrc/uvs_feature_reject.hip,
// csrc/uvs_feature_detect.hip); what is here is the bookkeeping around them.  Differences from the reference, all from the C ABI below:
// positions are FP64 (cv::Point2f there), setMask orders with a stable sort and keeps no image (the occupied points go to uvs_ft_detect, whose
// disc is Euclidean), rejectWithF works on the normalized points with F_THRESHOLD / FOCAL_LENGTH (the same test as on the reference's virtual
// image) and is off unless f_threshold > 0, CLAHE (EQUALIZE, :60-66) runs on the device inside uvs_ft_track when `equalize` is set, and n_id is
// a member, not a static, so that two trackers of one process number their points apart.  With max_cnt = 0 (the default) new points are the caller's, through a Detector.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "../csrc/uvs_camera_models.h"

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
    explicit FeatureTrackerBook(const uvs_kf_camera& camera) : camera_(camera), lift_(uvs_cam_pack(uvs_cam_pinhole(camera))) {}
    // any camera model (MEI, Kannala-Brandt, or the pinhole given as one): the points are lifted through uvs_cam_lift, the device function of
    // uvs_ft_lift.  Throws std::invalid_argument for a model the library would reject.
    explicit FeatureTrackerBook(const uvs_camera_model& model) : camera_{}, has_model_(true) {
        std::string err;
        if (uvs_cam_take(&model, "FeatureTrackerBook", err, &lift_) != UVS_OK) throw std::invalid_argument(err);
    }

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

    // :149-182 after findFundamentalMat: the six reduceVector calls by its status (keep[i] != 0 keeps track i), and the device's normalized
    // forward points alike.  keep has one entry per forward point; any other size changes nothing and returns false.
    bool applyReject(const std::vector<uint8_t>& keep) {
        if (keep.size() != forw_pts.size()) return false;
        const bool with_norm = forw_norm_.size() == forw_pts.size();
        if (prev_pts.size() <= keep.size()) reduceVector(prev_pts, keep);      // (longer than the tracks: the reference reads past its status there)
        reduceVector(cur_pts, keep); reduceVector(forw_pts, keep); reduceVector(cur_un_pts, keep);
        reduceVector(ids, keep); reduceVector(track_cnt, keep);
        if (with_norm) reduceVector(forw_norm_, keep);
        return true;
    }

    // :9-42.  The points are ordered by track_cnt descending (a STABLE sort: the reference's std::sort leaves the order of ties open), and a
    // point is kept iff no point kept before it lies within min_dist of it, dx^2 + dy^2 <= min_dist^2 on the rint centres (the filled cv::circle
    // of the reference's mask as a Euclidean disc).  forw_pts, ids, track_cnt and the device's normalized points are permuted alike.
    void setMask(int min_dist) {
        const size_t n = forw_pts.size();
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [this](size_t a, size_t b) { return track_cnt[a] > track_cnt[b]; });
        const bool with_norm = forw_norm_.size() == n;
        const long long r2 = (long long)min_dist * min_dist;
        std::vector<Point2d> pts, norm;
        std::vector<int> id, cnt;
        std::vector<long long> cx, cy;
        for (size_t i : order) {
            const long long x = (long long)std::nearbyint(forw_pts[i].x), y = (long long)std::nearbyint(forw_pts[i].y);
            bool keep = true;
            for (size_t k = 0; k < cx.size() && keep; ++k) keep = (x - cx[k]) * (x - cx[k]) + (y - cy[k]) * (y - cy[k]) > r2;
            if (!keep) continue;
            pts.push_back(forw_pts[i]); id.push_back(ids[i]); cnt.push_back(track_cnt[i]);
            if (with_norm) norm.push_back(forw_norm_[i]);
            cx.push_back(x); cy.push_back(y);
        }
        forw_pts.swap(pts); ids.swap(id); track_cnt.swap(cnt);
        if (with_norm) forw_norm_.swap(norm);
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
    // function (uvs_cam_lift of uvs_camera_models.h).  std::map::insert keeps the first entry of a key, as the reference's does for the ids still -1.
    void undistortedPoints() {
        cur_un_pts.clear(); cur_un_pts_map.clear();
        for (size_t i = 0; i < cur_pts.size(); ++i) {
            Point2d b;
            if (i < forw_norm_.size()) b = forw_norm_[i];
            else { double ray[3]; uvs_cam_lift(lift_, cur_pts[i].x, cur_pts[i].y, ray, b.x, b.y); }
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

    // :60-66, EQUALIZE.  The setting lives on the device, in the tracker's slot (uvs_ft_set_equalize), and is sent when it differs from what the
    // slot was last told; a fresh slot, and a slot after a reset, is plain.  FeatureTracker::readImage asks equalizePending() before every frame.
    bool equalizePending() const {
        if (!eq_told_) return equalize;
        return told_equalize_ != equalize || (equalize && (told_clip_ != clahe_clip || told_tiles_ != clahe_tiles));
    }
    void equalizeTold() { eq_told_ = true; told_equalize_ = equalize; told_clip_ = clahe_clip; told_tiles_ = clahe_tiles; }
    void equalizeForgotten() { eq_told_ = false; }      // the slot was reset

    bool equalize = false;            // EQUALIZE: readImage's images are raw and go through CLAHE on the device
    double clahe_clip = 3.0;          // cv::createCLAHE(3.0, cv::Size(8, 8))
    int clahe_tiles = 8;
    std::vector<Point2d> n_pts, prev_pts, cur_pts, forw_pts, prev_un_pts, cur_un_pts, pts_velocity;
    std::vector<int> ids, track_cnt;
    std::map<int, Point2d> cur_un_pts_map, prev_un_pts_map;
    double cur_time = 0.0, prev_time = 0.0;
    int n_id = 0;

protected:
    uvs_kf_camera camera_;
    UvsCamDev lift_ = uvs_cam_none(); // the camera or the model, packed: what undistortedPoints lifts through
    bool has_model_ = false;          // constructed from a uvs_camera_model: camera_ is not used
    const uvs_kf_camera* cameraArg() const { return has_model_ ? nullptr : &camera_; }      // the `camera` of uvs_ft_track / uvs_ft_detect
    std::vector<Point2d> forw_norm_;

private:
    bool eq_told_ = false, told_equalize_ = false;      // what the slot was last told
    double told_clip_ = 0.0;
    int told_tiles_ = 0;
};

class FeatureTracker : public FeatureTrackerBook {
public:
    // where goodFeaturesToTrack sits (:119-131): called with the tracker after the flow (forw_pts are the tracked points), fills n_pts
    using Detector = std::function<void(const FeatureTracker&, std::vector<Point2d>&)>;

    // throws std::runtime_error without a GPU (no CPU path)
    FeatureTracker(const uvs_kf_camera& camera, int device = 0, int max_width = 752, int max_height = 480, int levels = 4, int max_points = 1024)
        : FeatureTrackerBook(camera), max_points_(max_points) {
        const int rc = uvs_ft_create(device, 1, max_width, max_height, levels, max_points, &ft_);
        if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_ft_create: ") + uvs_status_string(rc));
    }
    // the same with a camera model on the device handle (uvs_ft_set_camera_model): undistortedPoints, pts_velocity, rejectWithF and the
    // tracker's own detection then run on model-lifted points
    FeatureTracker(const uvs_camera_model& model, int device = 0, int max_width = 752, int max_height = 480, int levels = 4, int max_points = 1024)
        : FeatureTrackerBook(model), max_points_(max_points) {
        int rc = uvs_ft_create(device, 1, max_width, max_height, levels, max_points, &ft_);
        if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_ft_create: ") + uvs_status_string(rc));
        if ((rc = uvs_ft_set_camera_model(ft_, &model)) != UVS_OK) {
            const std::string text = uvs_ft_last_error(ft_);
            uvs_ft_destroy(ft_);
            throw std::runtime_error("uvs_ft_set_camera_model: " + text);
        }
    }
    ~FeatureTracker() { uvs_ft_destroy(ft_); }
    FeatureTracker(const FeatureTracker&) = delete;
    FeatureTracker& operator=(const FeatureTracker&) = delete;

    // the reference's fisheye mask: detection is allowed where it is non-zero.  [height][width] of the images' size; it goes to the device
    // (uvs_ft_set_mask) with the next image and stays there.  nullptr clears it.
    void setImageMask(const uint8_t* mask, int width, int height) {
        if (mask) image_mask_.assign(mask, mask + (size_t)width * height); else image_mask_.clear();
        mask_w_ = width; mask_h_ = height; mask_pending_ = true;
    }

    // :54-147 with PUB_THIS_FRAME set.  image: [height][width] grey levels, the raw frame as in the reference: with `equalize` set the device
    // runs CLAHE (clahe_clip, clahe_tiles x clahe_tiles) on it before anything else sees it (:60-66).  Returns UVS_OK or the error
    // of uvs_ft_track (its text in last_error; the vectors are unchanged then).  Without a Detector and with max_cnt > 0 the frame goes on as
    // :109-139 does: setMask, uvs_ft_detect of max_cnt - forw_pts.size() points with the kept points occupied, addPoints; an error of the
    // detection is returned after the frame has been finished without new points.  With f_threshold > 0 rejectWithF (:111) runs between the
    // flow and setMask / the Detector, on frames that carry at least 8 tracks; an error of it is returned after the frame has been finished
    // with every track kept.
    int readImage(const uint8_t* image, int width, int height, double time, const Detector& detect = nullptr) {
        if (const int rc = pushEqualize()) return rc;
        const size_t n = cur_pts.size();
        xy_.resize(2 * n + 2); nxt_.resize(2 * n + 2); nrm_.resize(2 * n + 2); st_.resize(n + 1); it_.resize(n + 1);
        for (size_t i = 0; i < n; ++i) { xy_[2 * i] = cur_pts[i].x; xy_[2 * i + 1] = cur_pts[i].y; }
        uvs_ft_item item;
        item.image = image; item.stream = 0; item.width = width; item.height = height; item.n_points = (int32_t)n; item.points_xy = n ? xy_.data() : nullptr;
        int32_t n_tracked = 0;
        const int rc = uvs_ft_track(ft_, 1, &item, cameraArg(), nxt_.data(), st_.data(), it_.data(), nrm_.data(), &n_tracked);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        std::vector<Point2d> next(n), norm(n);
        for (size_t i = 0; i < n; ++i) { next[i].x = nxt_[2 * i]; next[i].y = nxt_[2 * i + 1]; norm[i].x = nrm_[2 * i]; norm[i].y = nrm_[2 * i + 1]; }
        applyFlow(time, next, std::vector<int32_t>(st_.begin(), st_.begin() + n), norm);
        const int rej_rc = f_threshold > 0.0 ? rejectWithF() : UVS_OK;
        ++frame_cnt_;
        n_pts.clear();
        int det_rc = UVS_OK;
        if (detect) detect(*this, n_pts);
        else if (max_cnt > 0) {
            setMask(min_dist);
            det_rc = detectNew();
        }
        addPoints();
        rotate();
        return rej_rc != UVS_OK ? rej_rc : det_rc;
    }

    int max_cnt = 0;                  // MAX_CNT; 0: new points are the Detector's
    int min_dist = 30;                // MIN_DIST
    double quality_level = 0.01;
    double f_threshold = 0.0;         // F_THRESHOLD in pixels of the virtual image; 0: rejectWithF is off
    double focal_length = 460.0;      // FOCAL_LENGTH
    uint64_t ransac_seed = 0;         // frame k (0, 1, ..) samples with ransac_seed + k
    uvs_ft_reject_result last_reject = {};      // of the last frame that ran rejectWithF
    std::string last_error;

    // empties the device slot (the next image may have another size; it must find no points here, so the vectors are emptied too); the slot's
    // equalization and mask are cleared with it and pushed again by the next frame
    int reset() {
        const int rc = uvs_ft_reset(ft_, 0);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        prev_pts.clear(); cur_pts.clear(); forw_pts.clear(); prev_un_pts.clear(); cur_un_pts.clear(); pts_velocity.clear(); ids.clear(); track_cnt.clear();
        forw_norm_.clear();
        equalizeForgotten();
        if (!image_mask_.empty()) mask_pending_ = true;
        return UVS_OK;
    }

private:
    // the equalization setting to the slot when it changed or the slot was reset (the way mask_pending_ works for the mask)
    int pushEqualize() {
        if (!equalizePending()) return UVS_OK;
        const int rc = uvs_ft_set_equalize(ft_, 0, clahe_clip, equalize ? clahe_tiles : 0, equalize ? clahe_tiles : 0);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        equalizeTold();
        return UVS_OK;
    }

    // :149-182: cur_un_pts and the device's normalized forward points through uvs_ft_reject, then the reduceVector calls
    int rejectWithF() {
        const size_t n = forw_pts.size();
        if (n < 8 || cur_un_pts.size() != n || forw_norm_.size() != n) return UVS_OK;
        xy_.resize(2 * n + 2); nrm_.resize(2 * n + 2);
        for (size_t i = 0; i < n; ++i) { xy_[2 * i] = cur_un_pts[i].x; xy_[2 * i + 1] = cur_un_pts[i].y; nrm_[2 * i] = forw_norm_[i].x; nrm_[2 * i + 1] = forw_norm_[i].y; }
        uvs_ft_reject_item item;
        item.n_points = (int32_t)n; item.reserved = 0; item.seed = ransac_seed + frame_cnt_; item.prev_norm = xy_.data(); item.next_norm = nrm_.data();
        std::vector<uint8_t> keep(n);
        const int rc = uvs_ft_reject(ft_, 1, &item, f_threshold / focal_length, 0.99, keep.data(), &last_reject);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        applyReject(keep);
        return UVS_OK;
    }

    // :119-131: fills n_pts and appends the device's normalized points, so that undistortedPoints uses them for the new points too
    int detectNew() {
        if (mask_pending_) {
            const int rc = uvs_ft_set_mask(ft_, 0, image_mask_.empty() ? nullptr : image_mask_.data(), mask_w_, mask_h_);
            if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
            mask_pending_ = false;
        }
        const int n_max_cnt = std::min(max_cnt - (int)forw_pts.size(), max_points_);
        if (n_max_cnt <= 0) return UVS_OK;
        const size_t n = forw_pts.size();
        xy_.resize(2 * n + 2);
        for (size_t i = 0; i < n; ++i) { xy_[2 * i] = forw_pts[i].x; xy_[2 * i + 1] = forw_pts[i].y; }
        uvs_ft_detect_item item;
        item.stream = 0; item.n_occupied = (int32_t)n; item.max_new = n_max_cnt; item.reserved = 0; item.occupied_xy = n ? xy_.data() : nullptr;
        new_xy_.resize(2 * (size_t)n_max_cnt); new_score_.resize(n_max_cnt); new_norm_.resize(2 * (size_t)n_max_cnt);
        uvs_ft_detect_result res;
        const int rc = uvs_ft_detect(ft_, 1, &item, quality_level, min_dist, cameraArg(), new_xy_.data(), new_score_.data(), new_norm_.data(), &res);
        if (rc != UVS_OK) { last_error = uvs_ft_last_error(ft_); return rc; }
        const bool with_norm = forw_norm_.size() == n;
        for (int i = 0; i < res.n_new; ++i) {
            Point2d p, m;
            p.x = (double)new_xy_[2 * i]; p.y = (double)new_xy_[2 * i + 1]; m.x = new_norm_[2 * i]; m.y = new_norm_[2 * i + 1];
            n_pts.push_back(p);
            if (with_norm) forw_norm_.push_back(m);
        }
        return UVS_OK;
    }

    int max_points_ = 0;
    uint64_t frame_cnt_ = 0;          // frames read
    std::vector<uint8_t> image_mask_;
    int mask_w_ = 0, mask_h_ = 0;
    bool mask_pending_ = false;
    std::vector<int32_t> new_xy_;
    std::vector<double> new_score_, new_norm_;
    uvs_ft_tracker* ft_ = nullptr;
    std::vector<double> xy_, nxt_, nrm_;
    std::vector<int32_t> st_, it_;
};

}  // namespace uvs
