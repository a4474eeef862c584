// feature_tracker_capi.cpp -- test hooks for uvs::FeatureTracker (feature_tracker.h): a tracker behind a handle, fed with images (the device
// path) or with a frame's flow results by hand (the bookkeeping alone, no device), and its vectors read back.  Apart from host_capi.cpp for the
// reason vanishing_points_capi.cpp gives: the CPU oracle has no uvs_ft_*.
//   camera[8] = fx, fy, cx, cy, k1, k2, p1, p2 (uvs_host_ft_create_model: any camera model instead); new_xy[n_new][2]: the points the caller's detector adds in this frame.
// uvs_host_ft_set_detection turns the tracker's own detection on (max_cnt > 0): uvs_host_ft_read_image_detect then runs a frame without a
// Detector, and uvs_host_ft_apply_set_mask a frame of the bookkeeping with setMask between the flow and addPoints.
// uvs_host_ft_set_rejection turns rejectWithF on (f_threshold > 0) for the frames that follow, and uvs_host_ft_apply_reject is a frame of the
// bookkeeping with a given keep mask between the flow and addPoints.
// uvs_host_ft_set_equalize sets EQUALIZE and its CLAHE parameters for the frames that follow; uvs_host_ft_reset empties the tracker.
#include <cstdio>
#include <memory>
#include "feature_tracker.h"

namespace {
struct HostFt {
    std::unique_ptr<uvs::FeatureTracker> dev;      // null: bookkeeping only
    std::unique_ptr<uvs::FeatureTrackerBook> book;
    uvs::FeatureTrackerBook& b() { return dev ? *dev : *book; }
};
std::vector<uvs::Point2d> points(int n, const double* xy) {
    std::vector<uvs::Point2d> v(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) { v[i].x = xy[2 * i]; v[i].y = xy[2 * i + 1]; }
    return v;
}
}  // namespace

extern "C" {

// device < 0: no device is touched, the handle takes uvs_host_ft_read_flow only
void* uvs_host_ft_create(int device, const double* camera, int max_width, int max_height, int levels, int max_points) {
    if (!camera) return nullptr;
    const uvs_kf_camera cam{camera[0], camera[1], camera[2], camera[3], camera[4], camera[5], camera[6], camera[7]};
    try {
        HostFt* h = new HostFt();
        if (device < 0) h->book.reset(new uvs::FeatureTrackerBook(cam));
        else h->dev.reset(new uvs::FeatureTracker(cam, device, max_width, max_height, levels, max_points));
        return h;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return nullptr;
    }
}

// the same from a camera model: model_id = UVS_CAM_*, params[n_params] in the order of uvs_camera_model.p
void* uvs_host_ft_create_model(int device, int model_id, int n_params, const double* params, int max_width, int max_height, int levels, int max_points) {
    if (!params || n_params < 0 || n_params > 12) return nullptr;
    uvs_camera_model model = {};
    model.model = model_id;
    for (int i = 0; i < n_params; ++i) model.p[i] = params[i];
    try {
        HostFt* h = new HostFt();
        if (device < 0) h->book.reset(new uvs::FeatureTrackerBook(model));
        else h->dev.reset(new uvs::FeatureTracker(model, device, max_width, max_height, levels, max_points));
        return h;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return nullptr;
    }
}

void uvs_host_ft_destroy(void* h) { delete static_cast<HostFt*>(h); }

int uvs_host_ft_read_image(void* hv, const unsigned char* image, int width, int height, double time, int n_new, const double* new_xy) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev || !image || n_new < 0 || (n_new > 0 && !new_xy)) return UVS_ERR_INVALID_ARG;
    const std::vector<uvs::Point2d> fresh = points(n_new, new_xy);
    const int rc = h->dev->readImage(image, width, height, time, [&](const uvs::FeatureTracker&, std::vector<uvs::Point2d>& n_pts) { n_pts = fresh; });
    if (rc != UVS_OK) std::fprintf(stderr, "uvs_host_ft_read_image: %s\n", h->dev->last_error.c_str());
    return rc;
}

// one frame of the bookkeeping from given flow results: next_xy[n][2], ft_status[n] (UVS_FT_*), next_norm[n][2], n = the points held
int uvs_host_ft_read_flow(void* hv, double time, int n, const double* next_xy, const int* ft_status, const double* next_norm, int n_new, const double* new_xy) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || n < 0 || n_new < 0 || (n > 0 && (!next_xy || !ft_status || !next_norm)) || (n_new > 0 && !new_xy)) return UVS_ERR_INVALID_ARG;
    uvs::FeatureTrackerBook& b = h->b();
    if ((size_t)n != b.cur_pts.size()) return UVS_ERR_INVALID_ARG;
    b.applyFlow(time, points(n, next_xy), std::vector<int32_t>(ft_status, ft_status + n), points(n, next_norm));
    b.n_pts = points(n_new, new_xy);
    b.addPoints();
    b.rotate();
    return UVS_OK;
}

// max_cnt, min_dist, quality_level of the tracker's own detection (a device handle)
int uvs_host_ft_set_detection(void* hv, int max_cnt, int min_dist, double quality_level) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev || max_cnt < 0) return UVS_ERR_INVALID_ARG;
    h->dev->max_cnt = max_cnt; h->dev->min_dist = min_dist; h->dev->quality_level = quality_level;
    return UVS_OK;
}

// the fisheye mask [height][width]; null clears it
int uvs_host_ft_set_image_mask(void* hv, const unsigned char* mask, int width, int height) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev) return UVS_ERR_INVALID_ARG;
    h->dev->setImageMask(mask, width, height);
    return UVS_OK;
}

// readImage without a Detector: with max_cnt > 0 the new points are uvs_ft_detect's
int uvs_host_ft_read_image_detect(void* hv, const unsigned char* image, int width, int height, double time) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev || !image) return UVS_ERR_INVALID_ARG;
    const int rc = h->dev->readImage(image, width, height, time);
    if (rc != UVS_OK) std::fprintf(stderr, "uvs_host_ft_read_image_detect: %s\n", h->dev->last_error.c_str());
    return rc;
}

// uvs_host_ft_read_flow with setMask(min_dist) between the flow and addPoints (the bookkeeping alone: no device is touched)
int uvs_host_ft_apply_set_mask(void* hv, double time, int n, const double* next_xy, const int* ft_status, const double* next_norm, int min_dist, int n_new,
                               const double* new_xy) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || n < 0 || n_new < 0 || min_dist < 0 || (n > 0 && (!next_xy || !ft_status || !next_norm)) || (n_new > 0 && !new_xy)) return UVS_ERR_INVALID_ARG;
    uvs::FeatureTrackerBook& b = h->b();
    if ((size_t)n != b.cur_pts.size()) return UVS_ERR_INVALID_ARG;
    b.applyFlow(time, points(n, next_xy), std::vector<int32_t>(ft_status, ft_status + n), points(n, next_norm));
    b.setMask(min_dist);
    b.n_pts = points(n_new, new_xy);
    b.addPoints();
    b.rotate();
    return UVS_OK;
}

// f_threshold (pixels at focal_length; 0 turns rejectWithF off), focal_length, ransac_seed of a device handle
int uvs_host_ft_set_rejection(void* hv, double f_threshold, double focal_length, unsigned long long ransac_seed) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev || !(f_threshold >= 0.0) || !(focal_length > 0.0)) return UVS_ERR_INVALID_ARG;
    h->dev->f_threshold = f_threshold; h->dev->focal_length = focal_length; h->dev->ransac_seed = ransac_seed;
    return UVS_OK;
}

// status, n_inliers, hypothesis, root, iterations of the last frame that ran rejectWithF (a device handle)
int uvs_host_ft_last_reject(void* hv, int* out5) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev || !out5) return UVS_ERR_INVALID_ARG;
    const uvs_ft_reject_result& r = h->dev->last_reject;
    out5[0] = r.status; out5[1] = r.n_inliers; out5[2] = r.hypothesis; out5[3] = r.root; out5[4] = r.iterations;
    return UVS_OK;
}

// uvs_host_ft_read_flow with applyReject(keep) between the flow and addPoints (the bookkeeping alone: no device is touched); keep[n_keep], n_keep
// = the points the flow left
int uvs_host_ft_apply_reject(void* hv, double time, int n, const double* next_xy, const int* ft_status, const double* next_norm, int n_keep,
                             const unsigned char* keep, int n_new, const double* new_xy) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || n < 0 || n_new < 0 || n_keep < 0 || (n > 0 && (!next_xy || !ft_status || !next_norm)) || (n_keep > 0 && !keep) || (n_new > 0 && !new_xy))
        return UVS_ERR_INVALID_ARG;
    uvs::FeatureTrackerBook& b = h->b();
    if ((size_t)n != b.cur_pts.size()) return UVS_ERR_INVALID_ARG;
    b.applyFlow(time, points(n, next_xy), std::vector<int32_t>(ft_status, ft_status + n), points(n, next_norm));
    const bool ok = b.applyReject(std::vector<uint8_t>(keep, keep + n_keep));
    b.n_pts = points(n_new, new_xy);
    b.addPoints();
    b.rotate();
    return ok ? UVS_OK : UVS_ERR_INVALID_ARG;
}

// EQUALIZE: the frames that follow are raw and go through CLAHE on the device (clip, tiles x tiles); equalize = 0: off.  Any handle: on one
// without a device only the bookkeeping of the setting runs (uvs_host_ft_equalize_pending, _told, _forgotten)
int uvs_host_ft_set_equalize(void* hv, int equalize, double clip, int tiles) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h) return UVS_ERR_INVALID_ARG;
    h->b().equalize = equalize != 0; h->b().clahe_clip = clip; h->b().clahe_tiles = tiles;
    return UVS_OK;
}

// 1 when readImage would send the setting to the slot before its next frame, 0 when the slot has it
int uvs_host_ft_equalize_pending(void* hv) {
    HostFt* h = static_cast<HostFt*>(hv);
    return h ? (h->b().equalizePending() ? 1 : 0) : -1;
}

// what readImage does after it sent the setting (told != 0), and what reset does (told == 0), by hand
int uvs_host_ft_equalize_told(void* hv, int told) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h) return UVS_ERR_INVALID_ARG;
    if (told) h->b().equalizeTold(); else h->b().equalizeForgotten();
    return UVS_OK;
}

// empties a device handle's slot and its vectors (uvs::FeatureTracker::reset)
int uvs_host_ft_reset(void* hv) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h || !h->dev) return UVS_ERR_INVALID_ARG;
    return h->dev->reset();
}

// updateID(i) for i = 0, 1, .. as the node does after readImage (feature_tracker_node.cpp); returns the number of points
int uvs_host_ft_update_ids(void* hv) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h) return -1;
    unsigned int i = 0;
    while (h->b().updateID(i)) ++i;
    return (int)i;
}

// copies up to `capacity` points out; returns the number held.  Any array may be null.
int uvs_host_ft_get(void* hv, int capacity, double* cur_pts, int* ids, int* track_cnt, double* cur_un_pts, double* pts_velocity) {
    HostFt* h = static_cast<HostFt*>(hv);
    if (!h) return -1;
    const uvs::FeatureTrackerBook& b = h->b();
    const int n = (int)b.cur_pts.size();
    for (int i = 0; i < n && i < capacity; ++i) {
        if (cur_pts) { cur_pts[2 * i] = b.cur_pts[i].x; cur_pts[2 * i + 1] = b.cur_pts[i].y; }
        if (ids) ids[i] = b.ids[i];
        if (track_cnt) track_cnt[i] = b.track_cnt[i];
        if (cur_un_pts) { cur_un_pts[2 * i] = b.cur_un_pts[i].x; cur_un_pts[2 * i + 1] = b.cur_un_pts[i].y; }
        if (pts_velocity) { pts_velocity[2 * i] = b.pts_velocity[i].x; pts_velocity[2 * i + 1] = b.pts_velocity[i].y; }
    }
    return n;
}

}  // extern "C"
