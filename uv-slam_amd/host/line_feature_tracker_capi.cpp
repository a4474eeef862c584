// line_feature_tracker_capi.cpp -- test hooks: uvs::LineFeatureTrackerBook fed by hand (no device) and uvs::LineFeatureTracker
// (line_feature_tracker.h) frame by frame, with the segments given or detected, and a stub whose detection is injected, so that a test can hold the host layer's ids, track counts and normalized end points to the
// reference's bookkeeping and to the direct uvs_lt_track() call.  Apart from host_capi.cpp for the reason vanishing_points_capi.cpp gives.
//   camera[4] = fx, fy, cx, cy; segments[n][4] pixels; prev_index[n] as uvs_lt_track returns it.
#include <cstdio>
#include "line_feature_tracker.h"

namespace {
// the bookkeeping with a detection given by hand: what the overload of readImage4Line without segments does once uvs_lt_detect_track has answered
struct StubBook : uvs::LineFeatureTrackerBook {
    using uvs::LineFeatureTrackerBook::LineFeatureTrackerBook;
    std::vector<double> next_seg; std::vector<int32_t> next_prev; int next_rc = UVS_OK; int finished = 0;
    int detectTrack(const uint8_t*, int, int, size_t& n) override {
        if (next_rc != UVS_OK) { n = 0; return next_rc; }
        det_seg = next_seg; det_prev_index = next_prev; n = next_prev.size();
        last_detect = uvs_lt_det_result{}; last_detect.n_found = last_detect.n_returned = (int32_t)n;
        return UVS_OK;
    }
    int finishFrame(size_t, const double*) override { ++finished; return UVS_OK; }
};
struct LtHook {
    std::unique_ptr<uvs::LineFeatureTrackerBook> book;      // the tracker when `tracker` is set
    uvs::LineFeatureTracker* tracker = nullptr;
    StubBook* stub = nullptr;                               // the book when made by uvs_host_lt_stub_create
};
}  // namespace

extern "C" {

// the bookkeeping alone: no device is touched
void* uvs_host_lt_book_create(const double* camera, int col_margin, int row_margin) {
    if (!camera) return nullptr;
    LtHook* h = new LtHook();
    h->book.reset(new uvs::LineFeatureTrackerBook(camera[0], camera[1], camera[2], camera[3], col_margin, row_margin));
    return h;
}

// the bookkeeping with uvs_host_lt_stub_inject standing in for the device's detection: no device is touched
void* uvs_host_lt_stub_create(const double* camera, int col_margin, int row_margin) {
    if (!camera) return nullptr;
    LtHook* h = new LtHook();
    h->stub = new StubBook(camera[0], camera[1], camera[2], camera[3], col_margin, row_margin);
    h->book.reset(h->stub);
    return h;
}

// what the next uvs_host_lt_read_image_detect finds: n segments with their prev_index, or the error rc
int uvs_host_lt_stub_inject(void* p, int rc, int n, const double* segments, const int32_t* prev_index) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->stub || n < 0 || (n > 0 && (!segments || !prev_index))) return UVS_ERR_INVALID_ARG;
    h->stub->next_rc = rc;
    h->stub->next_seg.assign(segments, segments + 4 * (size_t)n); h->stub->next_prev.assign(prev_index, prev_index + n);
    return UVS_OK;
}

// frames that reached finishFrame (a stub only)
int uvs_host_lt_stub_finished(void* p) {
    LtHook* h = static_cast<LtHook*>(p);
    return h && h->stub ? h->stub->finished : -1;
}

// the tracker on `device`; with_vp != 0 attaches the vanishing points with th_angle.  NULL without a GPU
void* uvs_host_lt_create(int device, const double* camera, int max_width, int max_height, int max_lines, int max_length, int col_margin,
                         int row_margin, int with_vp, double th_angle) {
    if (!camera) return nullptr;
    try {
        LtHook* h = new LtHook();
        h->tracker = new uvs::LineFeatureTracker(device, camera[0], camera[1], camera[2], camera[3], max_width, max_height, max_lines, max_length,
                                                 col_margin, row_margin);
        h->book.reset(h->tracker);
        if (with_vp) h->tracker->attachVanishingPoints(th_angle);
        return h;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return nullptr;
    }
}

void uvs_host_lt_destroy(void* p) { delete static_cast<LtHook*>(p); }

int uvs_host_lt_apply_matches(void* p, double time, int n, const double* segments, const int32_t* prev_index) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || n < 0 || (n > 0 && !segments)) return UVS_ERR_INVALID_ARG;
    h->book->applyMatches(time, (size_t)n, segments, prev_index);
    return UVS_OK;
}

int uvs_host_lt_read_image(void* p, const uint8_t* img, int width, int height, double time, int n, const double* segments) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->tracker || n < 0) return UVS_ERR_INVALID_ARG;
    const int rc = h->tracker->readImage4Line(img, width, height, (size_t)n, segments, time);
    if (rc != UVS_OK) std::fprintf(stderr, "uvs_host_lt_read_image: %s\n", h->tracker->last_error.c_str());
    return rc;
}

// uvs_lt_detect's parameters of a tracker's overload without segments
int uvs_host_lt_set_detect(void* p, int grad_threshold, int min_pixels, double min_length) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->tracker) return UVS_ERR_INVALID_ARG;
    h->tracker->grad_threshold = grad_threshold; h->tracker->min_pixels = min_pixels; h->tracker->min_length = min_length;
    return UVS_OK;
}

// setUndistortion(k1, k2, p1, p2) of a tracker: uvs_host_lt_read_image_detect then takes raw frames of the tracker's max_width x max_height
int uvs_host_lt_set_undistortion(void* p, double k1, double k2, double p1, double p2) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->tracker) return UVS_ERR_INVALID_ARG;
    return h->tracker->setUndistortion(k1, k2, p1, p2);
}

// setUndistortion(model, output pinhole) of a tracker: model_id = UVS_CAM_*, params[n_params] in the order of uvs_camera_model.p, out[4] = fx, fy, cx, cy
int uvs_host_lt_set_undistortion_model(void* p, int model_id, int n_params, const double* params, const double* out) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->tracker || !params || !out || n_params < 0 || n_params > 12) return UVS_ERR_INVALID_ARG;
    uvs_camera_model model = {};
    model.model = model_id;
    for (int i = 0; i < n_params; ++i) model.p[i] = params[i];
    return h->tracker->setUndistortion(model, out[0], out[1], out[2], out[3]);
}

// readImage4Line(img, width, height, time): the segments are detected (a tracker) or injected (a stub)
int uvs_host_lt_read_image_detect(void* p, const uint8_t* img, int width, int height, double time) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h) return UVS_ERR_INVALID_ARG;
    const int rc = h->book->readImage4Line(img, width, height, time);      // the plain bookkeeping has no detector: UVS_ERR_NO_DEVICE
    if (rc != UVS_OK && h->tracker) std::fprintf(stderr, "uvs_host_lt_read_image_detect: %s\n", h->tracker->last_error.c_str());
    return rc;
}

// the last detection of the overload without segments: returns n_returned; with capacity >= it, seg[n][4], width2[n], info[n][4],
// prev_index[n] are filled (each may be NULL); result[6] = status, n_found, n_returned, n_support, n_regions[2]
int uvs_host_lt_last_detect(void* p, int capacity, double* seg, double* width2, int32_t* info, int32_t* prev_index, int32_t* result) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h) return -1;
    const uvs::LineFeatureTrackerBook& b = *h->book;
    const int n = b.last_detect.n_returned;
    if (result) {
        result[0] = b.last_detect.status; result[1] = b.last_detect.n_found; result[2] = n; result[3] = b.last_detect.n_support;
        result[4] = b.last_detect.n_regions[0]; result[5] = b.last_detect.n_regions[1];
    }
    if (capacity < n) return n;
    for (int i = 0; i < n; ++i) {
        if (seg) for (int c = 0; c < 4; ++c) seg[4 * i + c] = b.det_seg[4 * i + c];
        if (width2) width2[i] = (size_t)i < b.det_width2.size() ? b.det_width2[i] : 0.0;
        if (info) for (int c = 0; c < 4; ++c) info[4 * i + c] = (size_t)(4 * i + c) < b.det_info.size() ? b.det_info[4 * i + c] : 0;
        if (prev_index) prev_index[i] = b.det_prev_index[i];
    }
    return n;
}

// updateID(i) for i = 0, 1, .. until it returns false, as the reference's caller loops; returns the number of lines
int uvs_host_lt_update_ids(void* p) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h) return -1;
    unsigned int i = 0;
    while (h->book->updateID(i)) ++i;
    return (int)i;
}

int uvs_host_lt_reset(void* p) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h) return UVS_ERR_INVALID_ARG;
    if (h->tracker) h->tracker->reset(); else h->book->reset();
    return UVS_OK;
}

// returns the number of lines; with capacity >= that number the arrays are filled: ids[n], track_cnt[n], pts[n][4] = curr start x, y, end
// x, y, un_pts[n][4] the same normalized, velocity[n][4], vps[n][3] (zero when no vanishing points are attached); any array may be NULL
int uvs_host_lt_get(void* p, int capacity, int32_t* ids, int32_t* track_cnt, double* pts, double* un_pts, double* velocity, double* vps) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h) return -1;
    const uvs::LineFeatureTrackerBook& b = *h->book;
    const int n = (int)b.ids.size();
    if (capacity < n) return n;
    for (int i = 0; i < n; ++i) {
        if (ids) ids[i] = b.ids[i];
        if (track_cnt) track_cnt[i] = b.track_cnt[i];
        if (pts) { pts[4 * i] = b.curr_start_pts[i].x; pts[4 * i + 1] = b.curr_start_pts[i].y; pts[4 * i + 2] = b.curr_end_pts[i].x; pts[4 * i + 3] = b.curr_end_pts[i].y; }
        if (un_pts) {
            un_pts[4 * i] = b.curr_start_un_pts[i].x; un_pts[4 * i + 1] = b.curr_start_un_pts[i].y;
            un_pts[4 * i + 2] = b.curr_end_un_pts[i].x; un_pts[4 * i + 3] = b.curr_end_un_pts[i].y;
        }
        if (velocity) {
            velocity[4 * i] = b.start_pts_velocity[i].x; velocity[4 * i + 1] = b.start_pts_velocity[i].y;
            velocity[4 * i + 2] = b.end_pts_velocity[i].x; velocity[4 * i + 3] = b.end_pts_velocity[i].y;
        }
        if (vps) for (int c = 0; c < 3; ++c) vps[3 * i + c] = (size_t)i < b.vps.size() ? b.vps[i](c) : 0.0;
    }
    return n;
}

// the last frame's device outputs of a tracker: desc[n][32], line_status[n], distance[n], and n_described / n_matched through result[2]
int uvs_host_lt_last(void* p, int n, uint8_t* desc, int32_t* line_status, int32_t* distance, int32_t* result) {
    LtHook* h = static_cast<LtHook*>(p);
    if (!h || !h->tracker || n < 0) return UVS_ERR_INVALID_ARG;
    const uvs::LineFeatureTracker& t = *h->tracker;
    if ((size_t)n * 32 > t.desc.size()) return UVS_ERR_CAPACITY;
    for (int i = 0; i < 32 * n; ++i) if (desc) desc[i] = t.desc[i];
    for (int i = 0; i < n; ++i) { if (line_status) line_status[i] = t.line_status[i]; if (distance) distance[i] = t.distance[i]; }
    if (result) { result[0] = t.last.n_described; result[1] = t.last.n_matched; }
    return UVS_OK;
}

}  // extern "C"
