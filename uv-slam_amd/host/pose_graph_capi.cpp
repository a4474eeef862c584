// pose_graph_capi.cpp -- test hook: a keyframe stream through the mirrored PoseGraph.
// Keyframes 0 .. n_before-1 are added (with their loops), optimize4DoF(cur_index) runs, then the rest are added (they take the drift);
// out_pose[n][7] = corrected (P, q x y z w) of every keyframe, out_drift[4] = (yaw_drift, t_drift), out_yaw_t[m][4] = the solve's raw output
// for the m keyframes first_looped_index .. cur_index (m returned through *out_m); tum_path (may be NULL) receives the corrected path.
// uvs_host_pose_graph_verify_run (below): the same stream with loop candidates instead of loops, verified on the GPU by findConnection.
// uvs_host_pose_graph_image_run: the same again from IMAGES: every keyframe extracts its own descriptors and keypoints on the GPU.
// uvs_host_pose_graph_detect_run (last): the verify run WITHOUT candidates: place recognition finds them on the GPU (addKeyFrameDetectLoop).
#include <cstdio>
#include <memory>
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

// Test hook: loop DETECTION through the mirrored PoseGraph.  Keyframe k carries its window points (n_query[k] of them: p3d[.][3] in its VIO
// frame, desc[.][4]) and its keypoints (n_kp[k]: uv_norm[.][2], kp_desc[.][4]), concatenated over k; candidate[k] = what detectLoop would
// return (-1: none).  Every keyframe goes through addKeyFrameWithCandidate (findConnection on the GPU); then optimize4DoF runs at the last
// keyframe with an accepted loop.  out_accepted[n], out_loop_info[n][8] (zeros without a loop), out_pose[n][7] = corrected (P, q x y z w).
extern "C" int uvs_host_pose_graph_verify_run(int device, int n, const double* stamps, const double* t, const double* q_xyzw, const int* sequence,
                                              const double* tic, const double* qic_xyzw, const int* n_query, const double* p3d, const uint64_t* desc,
                                              const int* n_kp, const double* uv_norm, const uint64_t* kp_desc, const int* candidate,
                                              int* out_accepted, double* out_loop_info, double* out_pose) {
    if (n < 1 || !stamps || !t || !q_xyzw || !sequence || !tic || !qic_xyzw || !n_query || !n_kp || !candidate || !out_accepted || !out_loop_info || !out_pose)
        return UVS_ERR_INVALID_ARG;
    try {
        PoseGraph graph(device, n, 256);
        graph.setExtrinsic(Eigen::Vector3d(tic[0], tic[1], tic[2]), Eigen::Quaterniond(qic_xyzw[3], qic_xyzw[0], qic_xyzw[1], qic_xyzw[2]));
        size_t qo = 0, ko = 0;
        int last_loop = -1;
        for (int k = 0; k < n; ++k) {
            const Eigen::Quaterniond Q(q_xyzw[4 * k + 3], q_xyzw[4 * k], q_xyzw[4 * k + 1], q_xyzw[4 * k + 2]);
            KeyFrame* kf = new KeyFrame(stamps[k], sequence[k], Eigen::Vector3d(t[3 * k], t[3 * k + 1], t[3 * k + 2]), Q.toRotationMatrix());
            for (int i = 0; i < n_query[k]; ++i, ++qo) {
                kf->point_3d.push_back(Eigen::Vector3d(p3d[3 * qo], p3d[3 * qo + 1], p3d[3 * qo + 2]));
                kf->point_id.push_back((double)i);
                kf->window_brief_descriptors.push_back({desc[4 * qo], desc[4 * qo + 1], desc[4 * qo + 2], desc[4 * qo + 3]});
            }
            for (int i = 0; i < n_kp[k]; ++i, ++ko) {
                kf->keypoints_norm.push_back({uv_norm[2 * ko], uv_norm[2 * ko + 1]});
                kf->brief_descriptors.push_back({kp_desc[4 * ko], kp_desc[4 * ko + 1], kp_desc[4 * ko + 2], kp_desc[4 * ko + 3]});
            }
            const bool acc = graph.addKeyFrameWithCandidate(kf, candidate[k]);
            if (kf->last_verify.reason < 0) { std::fprintf(stderr, "findConnection: uvs_lc_verify failed at keyframe %d\n", k); return UVS_ERR_INVALID_ARG; }
            out_accepted[k] = acc;
            for (int c = 0; c < 8; ++c) out_loop_info[8 * k + c] = acc ? kf->loop_info[c] : 0.0;
            if (acc) last_loop = kf->index;
        }
        if (last_loop >= 0) {
            const int rc = graph.optimize4DoF(last_loop);
            if (rc != UVS_OK) { std::fprintf(stderr, "optimize4DoF: %s\n", graph.last_error.c_str()); return rc; }
        }
        int k = 0;
        for (const KeyFrame* kf : graph.keyframelist) {
            const Eigen::Quaterniond Q(kf->R_w_i);
            const double v[7] = {kf->T_w_i.x(), kf->T_w_i.y(), kf->T_w_i.z(), Q.x(), Q.y(), Q.z(), Q.w()};
            for (int c = 0; c < 7; ++c) out_pose[7 * k + c] = v[c];
            ++k;
        }
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return UVS_ERR_NO_DEVICE;
    }
    return UVS_OK;
}

// Test hook: image to loop edge through the mirrored PoseGraph.  Keyframe k is built by the online constructor from images[k] (width x height
// grey levels) and its window points (n_query[k] of them: p3d[.][3] in its VIO frame, uv[.][2] pixels; concatenated over k), so its descriptors
// and keypoints come from uvs_kf_extract (pattern[4][256] = x1 | y1 | x2 | y2; a handle of max_keypoints); candidate[k] = what detectLoop would
// return (-1: none).  Every keyframe goes through addKeyFrameWithCandidate; then optimize4DoF runs at the last keyframe with an accepted loop.
// out_accepted[n], out_loop_info[n][8] (zeros without a loop), out_pose[n][7] = corrected (P, q x y z w), out_n_kp[n] = keypoints of
// keyframe k, out_kp_norm[n][max_keypoints][2] / out_kp_desc[n][max_keypoints][4] = its keypoints_norm / brief_descriptors,
// out_window_desc[.][4] = its window_brief_descriptors, concatenated over k.
extern "C" int uvs_host_pose_graph_image_run(int device, int n, const double* stamps, const double* t, const double* q_xyzw, const int* sequence,
                                             const double* tic, const double* qic_xyzw, const uvs_kf_camera* camera, const int32_t* pattern,
                                             int max_keypoints, int width, int height, const uint8_t* images, const int* n_query, const double* p3d,
                                             const float* uv, const int* candidate, int* out_accepted, double* out_loop_info, double* out_pose,
                                             int* out_n_kp, double* out_kp_norm, uint64_t* out_kp_desc, uint64_t* out_window_desc) {
    if (n < 1 || !stamps || !t || !q_xyzw || !sequence || !tic || !qic_xyzw || !camera || !pattern || !images || !n_query || !candidate || !out_accepted ||
        !out_loop_info || !out_pose || !out_n_kp || !out_kp_norm || !out_kp_desc || !out_window_desc)
        return UVS_ERR_INVALID_ARG;
    uvs_kf_extractor* kf = nullptr;
    int rc = uvs_kf_create(device, 1, width, height, max_keypoints, UVS_LC_MAX_QUERY, pattern, pattern + UVS_KF_PATTERN_BITS,
                           pattern + 2 * UVS_KF_PATTERN_BITS, pattern + 3 * UVS_KF_PATTERN_BITS, &kf);
    if (rc != UVS_OK) return rc;
    rc = UVS_OK;
    try {
        PoseGraph graph(device, n, 256);
        graph.setExtrinsic(Eigen::Vector3d(tic[0], tic[1], tic[2]), Eigen::Quaterniond(qic_xyzw[3], qic_xyzw[0], qic_xyzw[1], qic_xyzw[2]));
        size_t qo = 0;
        int last_loop = -1;
        for (int k = 0; k < n && rc == UVS_OK; ++k) {
            const Eigen::Quaterniond Q(q_xyzw[4 * k + 3], q_xyzw[4 * k], q_xyzw[4 * k + 1], q_xyzw[4 * k + 2]);
            std::vector<Eigen::Vector3d> point_3d;
            std::vector<std::array<float, 2>> point_2d_uv;
            std::vector<double> point_id;
            for (int i = 0; i < n_query[k]; ++i, ++qo) {
                point_3d.push_back(Eigen::Vector3d(p3d[3 * qo], p3d[3 * qo + 1], p3d[3 * qo + 2]));
                point_2d_uv.push_back({uv[2 * qo], uv[2 * qo + 1]});
                point_id.push_back((double)i);
            }
            KeyFrame* kfr = new KeyFrame(stamps[k], k, Eigen::Vector3d(t[3 * k], t[3 * k + 1], t[3 * k + 2]), Q.toRotationMatrix(),
                                         images + (size_t)k * width * height, width, height, point_3d, point_2d_uv, {}, point_id, sequence[k], kf, *camera);
            out_n_kp[k] = (int)kfr->keypoints_norm.size();
            for (size_t i = 0; i < kfr->keypoints_norm.size(); ++i) {
                const size_t o = (size_t)k * max_keypoints + i;
                for (int c = 0; c < 2; ++c) out_kp_norm[2 * o + c] = kfr->keypoints_norm[i][c];
                for (int c = 0; c < 4; ++c) out_kp_desc[4 * o + c] = kfr->brief_descriptors[i][c];
            }
            for (size_t i = 0; i < kfr->window_brief_descriptors.size(); ++i)
                for (int c = 0; c < 4; ++c) out_window_desc[4 * (qo - kfr->window_brief_descriptors.size() + i) + c] = kfr->window_brief_descriptors[i][c];
            const bool acc = graph.addKeyFrameWithCandidate(kfr, candidate[k]);      // the graph owns kfr from here
            if (kfr->last_verify.reason < 0) { std::fprintf(stderr, "findConnection: uvs_lc_verify failed at keyframe %d\n", k); rc = UVS_ERR_INVALID_ARG; break; }
            out_accepted[k] = acc;
            for (int c = 0; c < 8; ++c) out_loop_info[8 * k + c] = acc ? kfr->loop_info[c] : 0.0;
            if (acc) last_loop = kfr->index;
        }
        if (rc == UVS_OK && last_loop >= 0) {
            rc = graph.optimize4DoF(last_loop);
            if (rc != UVS_OK) std::fprintf(stderr, "optimize4DoF: %s\n", graph.last_error.c_str());
        }
        int k = 0;
        if (rc == UVS_OK)
            for (const KeyFrame* f : graph.keyframelist) {
                const Eigen::Quaterniond Q(f->R_w_i);
                const double v[7] = {f->T_w_i.x(), f->T_w_i.y(), f->T_w_i.z(), Q.x(), Q.y(), Q.z(), Q.w()};
                for (int c = 0; c < 7; ++c) out_pose[7 * k + c] = v[c];
                ++k;
            }
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = UVS_ERR_NO_DEVICE;
    }
    uvs_kf_destroy(kf);
    return rc;
}

// Test hook: the two online KeyFrame constructors on ONE extractor.  Keyframe k of n is built from images[k] (width x height) without window
// points, through the camera model (model_id = UVS_CAM_*, params[n_params] in the order of uvs_camera_model.p) where use_model[k] != 0 and
// through `camera` otherwise.  out_n_kp[n]; out_kp_xy[n][max_keypoints][2], out_kp_norm[n][max_keypoints][2] = its keypoints / keypoints_norm.
extern "C" int uvs_host_keyframe_online(int device, const uvs_kf_camera* camera, int model_id, int n_params, const double* params, const int32_t* pattern,
                                        int max_keypoints, int width, int height, int n, const uint8_t* images, const int* use_model, int* out_n_kp,
                                        int32_t* out_kp_xy, double* out_kp_norm) {
    if (n < 1 || !camera || !params || n_params < 0 || n_params > 12 || !pattern || !images || !use_model || !out_n_kp || !out_kp_xy || !out_kp_norm)
        return UVS_ERR_INVALID_ARG;
    uvs_camera_model model = {};
    model.model = model_id;
    for (int i = 0; i < n_params; ++i) model.p[i] = params[i];
    uvs_kf_extractor* kf = nullptr;
    int rc = uvs_kf_create(device, 1, width, height, max_keypoints, UVS_LC_MAX_QUERY, pattern, pattern + UVS_KF_PATTERN_BITS,
                           pattern + 2 * UVS_KF_PATTERN_BITS, pattern + 3 * UVS_KF_PATTERN_BITS, &kf);
    if (rc != UVS_OK) return rc;
    try {
        for (int k = 0; k < n; ++k) {
            const uint8_t* img = images + (size_t)k * width * height;
            const Eigen::Vector3d T(0.0, 0.0, 0.0);
            const Eigen::Matrix3d R = Eigen::Matrix3d::Identity();
            std::unique_ptr<KeyFrame> f(use_model[k] ? new KeyFrame((double)k, k, T, R, img, width, height, {}, {}, {}, {}, 0, kf, model)
                                                     : new KeyFrame((double)k, k, T, R, img, width, height, {}, {}, {}, {}, 0, kf, *camera));
            out_n_kp[k] = (int)f->keypoints_norm.size();
            for (size_t i = 0; i < f->keypoints_norm.size(); ++i) {
                const size_t o = (size_t)k * max_keypoints + i;
                for (int c = 0; c < 2; ++c) { out_kp_xy[2 * o + c] = f->keypoints[i][c]; out_kp_norm[2 * o + c] = f->keypoints_norm[i][c]; }
            }
        }
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = UVS_ERR_INVALID_ARG;
    }
    uvs_kf_destroy(kf);
    return rc;
}

// Test hook: place recognition through the mirrored PoseGraph.  The arguments of uvs_host_pose_graph_verify_run, with the vocabulary (the
// arguments of uvs_pr_create) in place of the candidates: every keyframe goes through addKeyFrameDetectLoop(kf, true), so detectLoop runs on
// the GPU and its answer goes to findConnection; then optimize4DoF runs at the last keyframe with an accepted loop.  out_candidate[n] = what
// detectLoop returned, the other outputs as uvs_host_pose_graph_verify_run's.
extern "C" int uvs_host_pose_graph_detect_run(int device, int n, const double* stamps, const double* t, const double* q_xyzw, const int* sequence,
                                              const double* tic, const double* qic_xyzw, const int* n_query, const double* p3d, const uint64_t* desc,
                                              const int* n_kp, const double* uv_norm, const uint64_t* kp_desc, int k, int L, int scoring_type,
                                              int weighting_type, int n_nodes, const int32_t* node_id, const int32_t* parent_id, const double* weight,
                                              const uint64_t* descriptor, int n_words, const int32_t* word_node_id, const int32_t* word_id,
                                              int* out_candidate, int* out_accepted, double* out_loop_info, double* out_pose) {
    if (n < 1 || !stamps || !t || !q_xyzw || !sequence || !tic || !qic_xyzw || !n_query || !n_kp || !out_candidate || !out_accepted || !out_loop_info || !out_pose)
        return UVS_ERR_INVALID_ARG;
    try {
        PoseGraph graph(device, n, 256);
        graph.setExtrinsic(Eigen::Vector3d(tic[0], tic[1], tic[2]), Eigen::Quaterniond(qic_xyzw[3], qic_xyzw[0], qic_xyzw[1], qic_xyzw[2]));
        graph.loadVocabulary(k, L, scoring_type, weighting_type, n_nodes, node_id, parent_id, weight, descriptor, n_words, word_node_id, word_id,
                             UVS_LC_MAX_OLD, 64);
        size_t qo = 0, ko = 0;
        int last_loop = -1;
        for (int f = 0; f < n; ++f) {
            const Eigen::Quaterniond Q(q_xyzw[4 * f + 3], q_xyzw[4 * f], q_xyzw[4 * f + 1], q_xyzw[4 * f + 2]);
            KeyFrame* kf = new KeyFrame(stamps[f], sequence[f], Eigen::Vector3d(t[3 * f], t[3 * f + 1], t[3 * f + 2]), Q.toRotationMatrix());
            for (int i = 0; i < n_query[f]; ++i, ++qo) {
                kf->point_3d.push_back(Eigen::Vector3d(p3d[3 * qo], p3d[3 * qo + 1], p3d[3 * qo + 2]));
                kf->point_id.push_back((double)i);
                kf->window_brief_descriptors.push_back({desc[4 * qo], desc[4 * qo + 1], desc[4 * qo + 2], desc[4 * qo + 3]});
            }
            for (int i = 0; i < n_kp[f]; ++i, ++ko) {
                kf->keypoints_norm.push_back({uv_norm[2 * ko], uv_norm[2 * ko + 1]});
                kf->brief_descriptors.push_back({kp_desc[4 * ko], kp_desc[4 * ko + 1], kp_desc[4 * ko + 2], kp_desc[4 * ko + 3]});
            }
            graph.last_error.clear();
            const bool acc = graph.addKeyFrameDetectLoop(kf, true);      // the graph owns kf from here
            if (!graph.last_error.empty()) { std::fprintf(stderr, "%s\n", graph.last_error.c_str()); return UVS_ERR_INVALID_ARG; }
            out_candidate[f] = graph.last_candidate;
            if (kf->last_verify.reason < 0) { std::fprintf(stderr, "findConnection: uvs_lc_verify failed at keyframe %d\n", f); return UVS_ERR_INVALID_ARG; }
            out_accepted[f] = acc;
            for (int c = 0; c < 8; ++c) out_loop_info[8 * f + c] = acc ? kf->loop_info[c] : 0.0;
            if (acc) last_loop = kf->index;
        }
        if (last_loop >= 0) {
            const int rc = graph.optimize4DoF(last_loop);
            if (rc != UVS_OK) { std::fprintf(stderr, "optimize4DoF: %s\n", graph.last_error.c_str()); return rc; }
        }
        int f = 0;
        for (const KeyFrame* kf : graph.keyframelist) {
            const Eigen::Quaterniond Q(kf->R_w_i);
            const double v[7] = {kf->T_w_i.x(), kf->T_w_i.y(), kf->T_w_i.z(), Q.x(), Q.y(), Q.z(), Q.w()};
            for (int c = 0; c < 7; ++c) out_pose[7 * f + c] = v[c];
            ++f;
        }
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return UVS_ERR_NO_DEVICE;
    }
    return UVS_OK;
}
