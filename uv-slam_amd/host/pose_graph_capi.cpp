// pose_graph_capi.cpp -- test hook: a keyframe stream through the mirrored PoseGraph.
// Keyframes 0 .. n_before-1 are added (with their loops), optimize4DoF(cur_index) runs, then the rest are added (they take the drift);
// out_pose[n][7] = corrected (P, q x y z w) of every keyframe, out_drift[4] = (yaw_drift, t_drift), out_yaw_t[m][4] = the solve's raw output
// for the m keyframes first_looped_index .. cur_index (m returned through *out_m); tum_path (may be NULL) receives the corrected path.
#include <cstdio>
#include <stdexcept>
#include "pose_graph.h"

extern "C" int uvs_host_pose_graph_run(int device, int n, const double* stamps, const double* t, const double* q_xyzw, const int* sequence,
                                       const int* loop_index, const double* loop_info, int n_before, int cur_index, const char* tum_path,
                                       double* out_pose, double* out_drift, uvs_pg_report* out_report) {
    if (n < 1 || n_before < 1 || n_before > n || cur_index < 0 || cur_index >= n_before) return UVS_ERR_INVALID_ARG;
    try {
        PoseGraph graph(device, n, 256);
        auto add = [&](int k) {
            const Eigen::Quaterniond Q(q_xyzw[4 * k + 3], q_xyzw[4 * k], q_xyzw[4 * k + 1], q_xyzw[4 * k + 2]);
            KeyFrame* kf = new KeyFrame(stamps[k], sequence[k], Eigen::Vector3d(t[3 * k], t[3 * k + 1], t[3 * k + 2]), Q.toRotationMatrix());
            LoopInfo li;
            for (int c = 0; c < 8; ++c) li[c] = loop_info[8 * k + c];
            graph.addKeyFrame(kf, loop_index[k], loop_index[k] >= 0 ? &li : nullptr);
        };
        for (int k = 0; k < n_before; ++k) add(k);
        const int rc = graph.optimize4DoF(cur_index);
        if (rc != UVS_OK) { std::fprintf(stderr, "optimize4DoF: %s\n", graph.last_error.c_str()); return rc; }
        if (out_report) *out_report = graph.last_report;
        out_drift[0] = graph.yaw_drift;
        for (int c = 0; c < 3; ++c) out_drift[1 + c] = graph.t_drift(c);
        for (int k = n_before; k < n; ++k) add(k);
        int k = 0;
        for (const KeyFrame* kf : graph.keyframelist) {
            const Eigen::Quaterniond Q(kf->R_w_i);
            const double v[7] = {kf->T_w_i.x(), kf->T_w_i.y(), kf->T_w_i.z(), Q.x(), Q.y(), Q.z(), Q.w()};
            for (int c = 0; c < 7; ++c) out_pose[7 * k + c] = v[c];
            ++k;
        }
        if (tum_path && !graph.writeTum(tum_path)) return UVS_ERR_INVALID_ARG;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return UVS_ERR_NO_DEVICE;
    }
    return UVS_OK;
}
