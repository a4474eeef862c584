// vanishing_points_capi.cpp -- test hook: one frame through uvs::VanishingPoints (vanishing_points.h), so that a test can show that the host
// layer returns the bits of the direct uvs_vp_estimate() call.  Apart from host_capi.cpp because that file is also compiled into the
// oracle-backed library (oracle/Makefile), and the CPU oracle has no uvs_vp_* (the estimator has no CPU path).
//   segments[n][4] pixels; camera[4] = fx, fy, cx, cy; messages_io[n][15]: line messages whose slots 12..14 are overwritten.
//   out_vps[3][3] = tmp_vps, out_ids[n] = local_vp_ids, out_result = the frame's uvs_vp_result.
#include <cstdio>
#include "feature_manager.h"
#include "vanishing_points.h"

extern "C" int uvs_host_vanishing_points(int device, int n, const double* segments, const double* camera, double th_angle, unsigned long long seed,
                                         double* messages_io, double* out_vps, int* out_ids, uvs_vp_result* out_result) {
    if (n < 0 || !camera || !out_vps || !out_ids || !out_result || (n > 0 && (!segments || !messages_io))) return UVS_ERR_INVALID_ARG;
    try {
        uvs::VanishingPoints vp(device, n > 0 ? n : 1);
        std::vector<uvs::KeyLineEnds> lines(n);
        for (int l = 0; l < n; ++l) lines[l] = {segments[4 * l], segments[4 * l + 1], segments[4 * l + 2], segments[4 * l + 3]};
        const uvs_vp_camera cam{camera[0], camera[1], camera[2], camera[3]};
        std::vector<Eigen::Vector3d> tmp_vps; std::vector<int> ids;
        const int rc = vp.estimate(lines, cam, th_angle, seed, tmp_vps, ids);
        if (rc != UVS_OK) { std::fprintf(stderr, "uvs_host_vanishing_points: %s\n", vp.last_error.c_str()); return rc; }
        std::vector<Eigen::Matrix<double, 15, 1>> msgs(n);
        for (int l = 0; l < n; ++l) for (int c = 0; c < 15; ++c) msgs[l](c) = messages_io[15 * l + c];
        vp.fillMessages(msgs);
        for (int l = 0; l < n; ++l) for (int c = 0; c < 15; ++c) messages_io[15 * l + c] = msgs[l](c);
        for (int k = 0; k < 3; ++k) { out_vps[3 * k] = tmp_vps[k].x(); out_vps[3 * k + 1] = tmp_vps[k].y(); out_vps[3 * k + 2] = tmp_vps[k].z(); }
        for (int l = 0; l < n; ++l) out_ids[l] = ids[l];
        *out_result = vp.last;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return UVS_ERR_NO_DEVICE;
    }
    return UVS_OK;
}
