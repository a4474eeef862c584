// uvs_ft_handle.h -- the handle behind the uvs_ft_* calls, shared by the four units of the point front end: csrc/uvs_feature_track.hip (creates
// and destroys it, builds the pyramids, tracks), csrc/uvs_feature_detect.hip (detects new points in level 0 of a slot's stored pyramid),
// csrc/uvs_feature_reject.hip (rejects outlier tracks by a fundamental-matrix RANSAC; it reads no slot) and csrc/uvs_feature_equalize.hip (CLAHE:
// of an equalized slot's raw image into level 0 of its new pyramid, on the tracking unit's behalf, and of loose images); csrc/uvs_camera_models.hip
// keeps the handle's camera model and lifts and projects loose points on its stream.  Device, stream, events
// and error text are the base's (uvs_handle.h, which also has align_up, pitch_of, the arena and the camera check the units use).  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/uvs_solver.h"
#include "uvs_camera_models.h"
#include "uvs_handle.h"

struct uvs_ft_tracker : UvsHandle {
    // cur: which of the slot's two pyramids is the stored one; has_mask: the slot's part of d_mask holds a mask (uvs_ft_set_mask);
    // equalize: the slot's images come raw and are equalized on the device with eq_* (uvs_ft_set_equalize).  uvs_ft_reset clears all of it
    struct Slot {
        int W = 0, H = 0, cur = 0; bool holds = false, has_mask = false;
        bool equalize = false; double eq_clip = 0.0; int eq_tiles_x = 0, eq_tiles_y = 0;
    };
    int max_streams = 0, max_width = 0, max_height = 0, levels = 0, max_points = 0;
    int max_candidates = UVS_FT_DEFAULT_CANDIDATES;      // uvs_ft_set_max_candidates
    float device_ms = 0.f, detect_ms = 0.f;     // uvs_ft_last_device_ms, uvs_ft_last_detect_device_ms
    std::vector<Slot> slots;
    size_t pyr_bytes = 0;                       // bytes of one pyramid at the largest size, every level rounded up to 256
    size_t img_slot = 0;                        // bytes of one level-0 image at the largest size, rounded up to 256
    size_t in_meta = 0;                         // bytes of (items | item of every point | points) at capacity, rounded up to 256
    DevBuf<uint8_t> d_pyr;                      // [max_streams][2] pyramids
    DevBuf<char> d_in, d_out;                   // the call's meta data / outputs (next_xy | next_norm | status | iterations | trace)
    PinnedBuf<char> h_in, h_out;                // pinned staging: meta data, then the repacked images / the outputs
    // detection (uvs_feature_detect.hip): allocated by the first call that needs them, so that a tracker that never detects pays nothing
    DevBuf<uint8_t> d_mask;                     // [max_streams] resident masks, each laid out as level 0 of a pyramid (first uvs_ft_set_mask)
    DevBuf<char> d_det;                         // one call's meta data, maps, candidate keys and outputs, sized by the images of the call
    PinnedBuf<char> h_det_in, h_det_out;        // pinned staging of uvs_ft_detect
    // outlier rejection (uvs_feature_reject.hip): allocated by the first call that needs them
    DevBuf<char> d_rej;                         // one call's item table and points, results and keep masks, and the debug arrays
    PinnedBuf<char> h_rej_in, h_rej_out;        // pinned staging of uvs_ft_reject
    float reject_ms = 0.f;                      // uvs_ft_last_reject_device_ms
    // equalization (uvs_feature_equalize.hip): allocated by the first call that needs them
    PinnedBuf<char> h_eq_in;                    // one call's job descriptors, then the raw images, each repacked to pitch_of rows
    DevBuf<char> d_eq_in;                       // ... on the device: the staging the kernels read
    DevBuf<uint8_t> d_eq_lut;                   // [job][tiles_y * tiles_x][256] LUTs of one call
    DevBuf<char> d_eq_out;                      // uvs_ft_equalize: the equalized images (pitch_of rows), then the debug call's bins
    PinnedBuf<char> h_eq_out;
    float equalize_ms = 0.f;                    // uvs_ft_last_equalize_device_ms
    // camera model (uvs_camera_models.hip): uvs_ft_set_camera_model's, which uvs_ft_track and uvs_ft_detect lift through while it is set
    // (model.model < 0: none; uvs_ft_reset keeps it), and the buffers of uvs_ft_lift / uvs_ft_project, allocated by the first call
    UvsCamDev model = uvs_cam_none();
    DevBuf<char> d_cm;                          // one call's points: (xy | ray | norm)
    PinnedBuf<char> h_cm;
};

namespace uvsft {

// sizes and byte offsets of the levels of one pyramid of a width x height image -> its bytes
inline size_t pyramid_layout(int width, int height, int levels, int* W, int* H, int* P, long long* off) {
    size_t bytes = 0;
    for (int l = 0; l < UVS_FT_MAX_LEVELS; ++l) {
        if (l < levels) {
            W[l] = l ? (W[l - 1] + 1) / 2 : width; H[l] = l ? (H[l - 1] + 1) / 2 : height; P[l] = pitch_of(W[l]);
            off[l] = (long long)bytes;
            bytes += align_up((size_t)P[l] * H[l], 256);
        } else { W[l] = H[l] = P[l] = 0; off[l] = 0; }
    }
    return bytes;
}

// ---- equalization: what uvs_feature_track.hip needs of uvs_feature_equalize.hip
// one image to equalize: the raw image on the host (stride = width) and where the result goes on the device (rows of dst_pitch bytes, dst and
// dst_pitch multiples of 4)
struct EqJob {
    const uint8_t* image; int width, height;
    double clip_limit; int tiles_x, tiles_y;
    uint8_t* dst; int dst_pitch;
};

// uploads the jobs' images in one copy and launches k_ft_clahe_lut and k_ft_clahe_apply on the handle's stream, without waiting; the caller has
// checked the arguments and set the device.  dbg_bins_dev: device memory for the bins of job 0 (uvs_ft_debug_equalize), or null
int equalize_enqueue(uvs_ft_tracker* h, int n, const EqJob* jobs, int32_t* dbg_bins_dev);

inline int check_equalize(double clip_limit, int tiles_x, int tiles_y, const std::string& fn, std::string& err) {
    if (!std::isfinite(clip_limit) || clip_limit < 0.0 || clip_limit > 256.0) { err = fn + ": clip_limit must be finite and in 0 .. 256"; return UVS_ERR_INVALID_ARG; }
    if (tiles_x < 1 || tiles_x > UVS_FT_CLAHE_MAX_TILES || tiles_y < 1 || tiles_y > UVS_FT_CLAHE_MAX_TILES) {
        err = fn + ": tiles_x and tiles_y must be 1 .. UVS_FT_CLAHE_MAX_TILES"; return UVS_ERR_INVALID_ARG;
    }
    return UVS_OK;
}

}  // namespace uvsft
