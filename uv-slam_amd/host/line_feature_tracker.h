// line_feature_tracker.h -- the reference's line front end after segment detection (feature_tracker/src/line_feature_tracker.cpp:351-433,
// 449-488: the ids and track counts of readImage4Line; :1140-1159 normalizePoints; :1205-1217 updateID) in the reference's own terms, above
// uvs_lt_track() and uvs_lt_detect_track(): an image, with or without its segments, in, ids / track_cnt / curr_start_pts / curr_end_pts / the normalized end points out.  Header-only.
// The descriptors (lineBiDes->compute) and lineMatching are on the GPU (csrc/uvs_line_track.hip); what is here is the bookkeeping around them.
// Differences from the reference, all from the C ABI below: the segments are the caller's detector's or, through the overload without
// segments, uvs_lt_detect's line-support regions (ELSED is not part of this library, and not in the reference tree), positions are FP64
// (cv::Point2f there), and n_id is a member, not a static, so that two trackers of one process number their lines apart.  The image is already
// undistorted and cropped, unless setUndistortion() was called: then the overload of readImage4Line without segments takes the raw frame, as
// the reference's does (:35-47), and the device undistorts and crops it (uvs_lt_set_undistort).  The overload with the caller's segments always
// takes the image those segments were found in.  With a uvs::VanishingPoints attached, `vps` is filled per line as :379-385 does.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "vanishing_points.h"

namespace uvs {

struct LinePoint2d { double x = 0.0, y = 0.0; };

// The bookkeeping of readImage4Line without the device: what happens to the vectors once the matches of a frame are known.
// LineFeatureTracker below feeds it from uvs_lt_track; a test may feed it by hand.
class LineFeatureTrackerBook {
public:
    // the pinhole camera of liftProjective4line (no distortion: the line image is undistorted); col_margin / row_margin: the reference's
    // cx -= COL_MARGIN, cy -= ROW_MARGIN for a cropped image (readIntrinsicParameter :1196-1202), 0 for none
    LineFeatureTrackerBook(double fx, double fy, double cx, double cy, int col_margin = 0, int row_margin = 0)
        : fx_(fx), fy_(fy), cx_(cx - col_margin), cy_(cy - row_margin) {
        inv_K11_ = 1.0 / fx_; inv_K13_ = -cx_ / fx_; inv_K22_ = 1.0 / fy_; inv_K23_ = -cy_ / fy_;
    }
    virtual ~LineFeatureTrackerBook() = default;

    // the gate points of a segment as the header states them: the ends ordered by x (a tie keeps them), truncated towards zero.  The reference
    // stores these in the KeyLine, and getStartPoint() / getEndPoint() return them
    static void gatePoints(const double* seg, LinePoint2d& s, LinePoint2d& e) {
        double sx = seg[0], sy = seg[1], ex = seg[2], ey = seg[3];
        if (sx > ex) { const double tx = sx, ty = sy; sx = ex; sy = ey; ex = tx; ey = ty; }
        s.x = (double)(int)sx; s.y = (double)(int)sy; e.x = (double)(int)ex; e.y = (double)(int)ey;
    }

    // :351-433 (and :449-488 for a first frame, where prev_index is all -1): segments[n][4]; prev_index[n] = for each new line the index of
    // the previous line it continues, or -1 (uvs_lt_track's prev_index: the reference walks good_match_vector in query order, so the LAST
    // query that chose a train line sets its id).  An index outside the previous lines counts as -1.
    void applyMatches(double time, size_t n, const double* segments, const int32_t* prev_index) {
        cur_time = time;
        std::vector<int> tmp_ids(n, -1), tmp_track_cnt(n, 1);
        curr_start_pts.assign(n, LinePoint2d()); curr_end_pts.assign(n, LinePoint2d());
        start_pts_velocity.assign(n, LinePoint2d()); end_pts_velocity.assign(n, LinePoint2d());
        vps.clear();
        for (size_t i = 0; i < n; ++i) {
            gatePoints(segments + 4 * i, curr_start_pts[i], curr_end_pts[i]);
            const int32_t q = prev_index ? prev_index[i] : -1;
            if (q >= 0 && (size_t)q < ids.size()) { tmp_ids[i] = ids[q]; tmp_track_cnt[i] = track_cnt[q] + 1; }
        }
        ids = tmp_ids; track_cnt = tmp_track_cnt;
        prev_start_un_pts = curr_start_un_pts; prev_end_un_pts = curr_end_un_pts;
        normalizePoints();
    }

    // :1140-1159 with liftProjective4line (PinholeCamera.cc:512-525): mx = inv_K11 x + inv_K13, my = inv_K22 y + inv_K23, each divided by z = 1
    void normalizePoints() {
        const size_t n = curr_start_pts.size();
        curr_start_un_pts.assign(n, LinePoint2d()); curr_end_un_pts.assign(n, LinePoint2d());
        for (size_t i = 0; i < n; ++i) {
            curr_start_un_pts[i] = lift(curr_start_pts[i]);
            curr_end_un_pts[i] = lift(curr_end_pts[i]);
        }
    }

    // :1205-1217
    bool updateID(unsigned int i) {
        if (i < ids.size()) {
            if (ids[i] == -1) ids[i] = n_id++;
            return true;
        }
        return false;
    }

    // One frame WITHOUT segments: detectTrack() finds and matches them (on the device in LineFeatureTracker; a test may override it and give
    // them by hand), then the bookkeeping above and finishFrame() (the vanishing points of LineFeatureTracker).  Returns detectTrack's or
    // finishFrame's error; after the former the frame changes nothing.
    int readImage4Line(const uint8_t* img, int width, int height, double time) {
        size_t n = 0;
        const int rc = detectTrack(img, width, height, n);
        if (rc != UVS_OK) return rc;
        applyMatches(time, n, det_seg.data(), det_prev_index.data());
        return finishFrame(n, det_seg.data());
    }

    void reset() {
        ids.clear(); track_cnt.clear(); curr_start_pts.clear(); curr_end_pts.clear(); curr_start_un_pts.clear(); curr_end_un_pts.clear();
        prev_start_un_pts.clear(); prev_end_un_pts.clear(); start_pts_velocity.clear(); end_pts_velocity.clear(); vps.clear();
    }

    std::vector<int> ids, track_cnt;
    std::vector<LinePoint2d> curr_start_pts, curr_end_pts, curr_start_un_pts, curr_end_un_pts, prev_start_un_pts, prev_end_un_pts;
    std::vector<LinePoint2d> start_pts_velocity, end_pts_velocity;      // zero, as the reference leaves them
    std::vector<Eigen::Vector3d> vps;                                   // per line, when a VanishingPoints is attached
    double cur_time = 0.0;
    int n_id = 0;
    // the last frame of the overload without segments: seg[n][4], width2[n], info[n][4] as uvs_lt_detect returns them, and the matches
    std::vector<double> det_seg, det_width2;
    std::vector<int32_t> det_info, det_prev_index;
    uvs_lt_det_result last_detect{};

protected:
    // fills det_seg, det_width2, det_info, det_prev_index and last_detect for the image; n = the lines returned
    virtual int detectTrack(const uint8_t*, int, int, size_t& n) { n = 0; return UVS_ERR_NO_DEVICE; }
    virtual int finishFrame(size_t, const double*) { return UVS_OK; }
    LinePoint2d lift(const LinePoint2d& p) const {
        const double mx = inv_K11_ * p.x + inv_K13_, my = inv_K22_ * p.y + inv_K23_, z = 1.0;
        LinePoint2d o;
        o.x = mx / z; o.y = my / z;
        return o;
    }
    double fx_, fy_, cx_, cy_, inv_K11_, inv_K13_, inv_K22_, inv_K23_;
};

class LineFeatureTracker : public LineFeatureTrackerBook {
public:
    // throws std::runtime_error without a GPU (no CPU path)
    LineFeatureTracker(int device, double fx, double fy, double cx, double cy, int max_width, int max_height, int max_lines = 256,
                       int max_length = UVS_LT_MAX_LENGTH, int col_margin = 0, int row_margin = 0)
        : LineFeatureTrackerBook(fx, fy, cx, cy, col_margin, row_margin), device_(device), max_lines_(max_lines), raw_fx_(fx), raw_fy_(fy), raw_cx_(cx),
          raw_cy_(cy), max_width_(max_width), max_height_(max_height), col_margin_(col_margin), row_margin_(row_margin) {
        const int rc = uvs_lt_create(device, 1, max_width, max_height, max_lines, max_length, &lt_);
        if (rc != UVS_OK) throw std::runtime_error(std::string("uvs_lt_create: ") + uvs_status_string(rc));
    }
    ~LineFeatureTracker() { uvs_lt_destroy(lt_); }
    LineFeatureTracker(const LineFeatureTracker&) = delete;
    LineFeatureTracker& operator=(const LineFeatureTracker&) = delete;

    // :86-91, :379-385: from now on every frame with more than one line estimates its vanishing points and fills `vps`
    void attachVanishingPoints(double thAngle) {
        vp_.reset(new VanishingPoints(device_, max_lines_));
        th_angle_ = thAngle;
    }

    // :1161-1188 imageUndistortion and the crop of :43-47, on the device: from now on readImage4Line(img, width, height, cur_time) takes the RAW
    // frame of width x height (0: the constructor's max_width x max_height, the reference's COL x ROW).  The map is built from the UNSHIFTED
    // fx, fy, cx, cy and the constructor's margins; the bookkeeping's shifted cx, cy then fit the cropped image.  Every parameter is rounded
    // through float first: the reference fills CV_32F matrices with them (:1168-1177), and cv::undistort works from those.
    // Returns UVS_OK or uvs_lt_set_undistort's error (its text in last_error; the map stays as it was).
    int setUndistortion(double k1, double k2, double p1, double p2, int width = 0, int height = 0) {
        const auto f32 = [](double v) { return (double)(float)v; };
        const uvs_kf_camera cam{f32(raw_fx_), f32(raw_fy_), f32(raw_cx_), f32(raw_cy_), f32(k1), f32(k2), f32(p1), f32(p2)};
        const int rc = uvs_lt_set_undistort(lt_, 0, &cam, width > 0 ? width : max_width_, height > 0 ? height : max_height_, col_margin_, row_margin_);
        if (rc != UVS_OK) last_error = uvs_lt_last_error(lt_);
        return rc;
    }
    // The same for a raw frame of any camera model (a fisheye: MEI, Kannala-Brandt): the device builds the map that takes the output pinhole
    // (fx_out, fy_out, cx_out, cy_out) of the uncropped undistorted image to the model's raw pixels (uvs_lt_set_undistort_model), cropped by the
    // constructor's margins.  The tracker itself should have been constructed with that output pinhole: it is the camera of the image the
    // lines are found in.  Nothing is rounded through float here: the reference has no such path to follow.
    int setUndistortion(const uvs_camera_model& model, double fx_out, double fy_out, double cx_out, double cy_out, int width = 0, int height = 0) {
        const int rc = uvs_lt_set_undistort_model(lt_, 0, &model, width > 0 ? width : max_width_, height > 0 ? height : max_height_, col_margin_,
                                                  row_margin_, fx_out, fy_out, cx_out, cy_out);
        if (rc != UVS_OK) last_error = uvs_lt_last_error(lt_);
        return rc;
    }

    // One frame: img[height][width] (undistorted, 8 bit), segments[n][4] = sx, sy, ex, ey of the caller's detector.  Returns UVS_OK or the
    // error of uvs_lt_track (its text in last_error; the frame changes nothing) or of uvs_vp_estimate (the lines are tracked, `vps` stays empty).
    int readImage4Line(const uint8_t* img, int width, int height, size_t n, const double* segments, double cur_time) {
        desc.assign(32 * n + 32, 0); line_status.assign(n + 1, 0); prev_index_.assign(n + 1, -1); distance.assign(n + 1, -1);
        uvs_lt_item it;
        it.image = img; it.stream = 0; it.width = width; it.height = height; it.n_lines = (int32_t)n; it.segments = segments;
        const int rc = uvs_lt_track(lt_, 1, &it, desc.data(), line_status.data(), prev_index_.data(), distance.data(), &last);
        if (rc != UVS_OK) { last_error = uvs_lt_last_error(lt_); return rc; }
        applyMatches(cur_time, n, segments, prev_index_.data());
        return finishFrame(n, segments);
    }
    using LineFeatureTrackerBook::readImage4Line;      // (img, width, height, cur_time): uvs_lt_detect_track finds the segments; after
                                                       // setUndistortion img is the raw frame and the segments are those of the undistorted one

    void reset() { LineFeatureTrackerBook::reset(); (void)uvs_lt_reset(lt_, 0); }

    uvs_lt_result last{};
    std::vector<uint8_t> desc;               // [n][32] of the last frame
    std::vector<int32_t> line_status, distance;
    std::string last_error;
    // uvs_lt_detect's parameters for the overload without segments
    int grad_threshold = 40, min_pixels = 10;
    double min_length = 12.0;

protected:
    int detectTrack(const uint8_t* img, int width, int height, size_t& n) override {
        const size_t m = (size_t)max_lines_;
        det_seg.assign(4 * m, 0.0); det_width2.assign(m, 0.0); det_info.assign(4 * m, 0); det_prev_index.assign(m + 1, -1);
        desc.assign(32 * m + 32, 0); line_status.assign(m + 1, 0); distance.assign(m + 1, -1);
        uvs_lt_det_item it;
        it.image = img; it.stream = 0; it.width = width; it.height = height; it.reserved = 0;
        uvs_lt_det_params pr;
        pr.grad_threshold = grad_threshold; pr.min_pixels = min_pixels; pr.min_length = min_length;
        const int rc = uvs_lt_detect_track(lt_, 1, &it, &pr, det_seg.data(), det_width2.data(), det_info.data(), &last_detect, desc.data(),
                                           line_status.data(), det_prev_index.data(), distance.data(), &last);
        if (rc != UVS_OK) { last_error = uvs_lt_last_error(lt_); n = 0; return rc; }
        n = (size_t)last_detect.n_returned;
        return UVS_OK;
    }

    // :379-385
    int finishFrame(size_t n, const double* segments) override {
        int rc = UVS_OK;
        if (vp_ && n > 1) {
            std::vector<KeyLineEnds> lines(n);
            for (size_t l = 0; l < n; ++l) lines[l] = {segments[4 * l], segments[4 * l + 1], segments[4 * l + 2], segments[4 * l + 3]};
            const uvs_vp_camera cam{fx_, fy_, cx_, cy_};
            std::vector<Eigen::Vector3d> tmp_vps; std::vector<int> local_vp_ids;
            rc = vp_->estimate(lines, cam, th_angle_, ++frame_, tmp_vps, local_vp_ids);
            if (rc != UVS_OK) { last_error = vp_->last_error; return rc; }
            vps.resize(n);
            for (size_t l = 0; l < n; ++l) vps[l] = vp_->lineVp(l);
        }
        return UVS_OK;
    }

private:
    uvs_lt_tracker* lt_ = nullptr;
    std::unique_ptr<VanishingPoints> vp_;
    std::vector<int32_t> prev_index_;
    double th_angle_ = 0.0;
    uint64_t frame_ = 0;
    int device_, max_lines_;
    double raw_fx_, raw_fy_, raw_cx_, raw_cy_;         // as given, before the margins' shift
    int max_width_, max_height_, col_margin_, row_margin_;
};

}  // namespace uvs
