// triangulate_capi.cpp -- test hooks for the device route of the host mirror (feature_manager.h: FeatureManager::tri, Estimator::setDeviceTriangulation).
// uvs_host_triangulate_device: FeatureManager::triangulate / triangulateLine through a uvs_tri handle of its own (one uvs_tri_triangulate call per
// member), with the arguments of uvs_host_triangulate (host_capi.cpp).  Apart from host_capi.cpp because that file is also compiled into the
// oracle-backed library (oracle/Makefile), and the CPU oracle has no uvs_tri_*.
#include <cstdio>
#include "estimator.h"
#include "triangulate_hook.h"

extern "C" int uvs_host_triangulate_device(const double* poses, const double* ex, int n_pt, const int* pt_start, const int* pt_nobs, const double* pt_obs,
                                           int n_ln, const int* ln_start, const int* ln_nobs, const double* ln_sp, const double* ln_ep,
                                           double* depth_io, double* orth_io) {
    uvs_tri* tri = nullptr;
    int rc = uvs_tri_create(0, 1, n_pt > 0 ? n_pt : 1, n_pt > 0 ? n_pt * (WINDOW_SIZE + 1) : 2, n_ln > 0 ? n_ln : 1, &tri);
    if (rc != UVS_OK) { std::fprintf(stderr, "uvs_host_triangulate_device: uvs_tri_create: %s\n", uvs_status_string(rc)); return rc; }
    try {
        rc = uvs_host_triangulate_with(tri, poses, ex, n_pt, pt_start, pt_nobs, pt_obs, n_ln, ln_start, ln_nobs, ln_sp, ln_ep, depth_io, orth_io);
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "uvs_host_triangulate_device: %s\n", e.what());
        rc = UVS_ERR_HIP;
    }
    uvs_tri_destroy(tri);
    return rc;
}

// The other two members with a device route, on flat arrays, by the host loop (use_device == 0) or through a uvs_tri handle:
//   setLineOrtho on n_ln lines of LINE_WINDOW views whose first view is (ln_sp0, ln_ep0), OLD parameters orth_old, NEW ones orth_new
//     -> flag_out[n_ln] = solve_flag, orth_out[n_ln][4] = orthonormal_vec afterwards;
//   removeBackShiftDepth on n_pt points anchored in frame 0 with three views (uv0, then uv1 twice) and depth_io[n_pt], between the camera
//     poses (marg_R[9], marg_P[3]) and (new_R[9], new_P[3]) -> depth_io.
extern "C" int uvs_host_check_and_shift(int use_device, const double* poses, const double* ex, int n_ln, const int* ln_start, const double* ln_sp0,
                                        const double* ln_ep0, const double* orth_old, const double* orth_new, int* flag_out, double* orth_out,
                                        int n_pt, const double* uv0, const double* uv1, double* depth_io, const double* marg_R, const double* marg_P,
                                        const double* new_R, const double* new_P) {
    setEurocParameters();
    Eigen::Vector3d Ps[WINDOW_SIZE + 1]; Eigen::Matrix3d Rs[WINDOW_SIZE + 1];
    for (int i = 0; i <= WINDOW_SIZE; ++i) {
        Ps[i] = Eigen::Vector3d(poses[7 * i], poses[7 * i + 1], poses[7 * i + 2]);
        Rs[i] = Eigen::Quaterniond(poses[7 * i + 6], poses[7 * i + 3], poses[7 * i + 4], poses[7 * i + 5]).toRotationMatrix();
    }
    const Eigen::Vector3d tic(ex[0], ex[1], ex[2]);
    const Eigen::Matrix3d ric = Eigen::Quaterniond(ex[6], ex[3], ex[4], ex[5]).toRotationMatrix();
    uvs_tri* tri = nullptr;
    if (use_device) {
        const int rc = uvs_tri_create(0, 1, n_pt > 0 ? n_pt : 1, 2, n_ln > 0 ? n_ln : 1, &tri);
        if (rc != UVS_OK) { std::fprintf(stderr, "uvs_host_check_and_shift: uvs_tri_create: %s\n", uvs_status_string(rc)); return rc; }
        uvs_tri_set_init_depth(tri, INIT_DEPTH);
    }
    int rc = 0;
    try {
        FeatureManager fm(Rs);
        fm.tri = tri;
        std::vector<Eigen::Vector4d> ortho;
        for (int l = 0; l < n_ln; ++l) {
            LineFeaturePerId f(l, ln_start[l]);
            LineFeaturePerFrame pf;
            pf.start_point = Eigen::Vector3d(ln_sp0[3 * l], ln_sp0[3 * l + 1], ln_sp0[3 * l + 2]); pf.end_point = Eigen::Vector3d(ln_ep0[3 * l], ln_ep0[3 * l + 1], ln_ep0[3 * l + 2]);
            f.line_feature_per_frame.assign(LINE_WINDOW, pf);
            f.orthonormal_vec = Eigen::Vector4d(orth_old[4 * l], orth_old[4 * l + 1], orth_old[4 * l + 2], orth_old[4 * l + 3]);
            fm.line_feature.push_back(f);
            ortho.emplace_back(orth_new[4 * l], orth_new[4 * l + 1], orth_new[4 * l + 2], orth_new[4 * l + 3]);
        }
        fm.setLineOrtho(ortho, Ps, Rs, tic, ric);
        int l = 0;
        for (auto& it : fm.line_feature) { flag_out[l] = it.solve_flag; for (int q = 0; q < 4; ++q) orth_out[4 * l + q] = it.orthonormal_vec[q]; ++l; }
        for (int k = 0; k < n_pt; ++k) {
            FeaturePerId f(k, 0);
            f.feature_per_frame.emplace_back(Eigen::Vector3d(uv0[3 * k], uv0[3 * k + 1], uv0[3 * k + 2]));
            for (int q = 0; q < 2; ++q) f.feature_per_frame.emplace_back(Eigen::Vector3d(uv1[3 * k], uv1[3 * k + 1], uv1[3 * k + 2]));
            f.estimated_depth = depth_io[k];
            fm.feature.push_back(f);
        }
        Eigen::Matrix3d mR, nR;
        for (int q = 0; q < 9; ++q) { mR(q / 3, q % 3) = marg_R[q]; nR(q / 3, q % 3) = new_R[q]; }
        fm.removeBackShiftDepth(mR, Eigen::Vector3d(marg_P[0], marg_P[1], marg_P[2]), nR, Eigen::Vector3d(new_P[0], new_P[1], new_P[2]));
        int k = 0;
        for (auto& it : fm.feature) { if (it.feature_per_frame.size() != 2 || it.start_frame != 0) rc = -2; depth_io[k++] = it.estimated_depth; }
        if (k != n_pt) rc = -3;
    } catch (const std::runtime_error& e) {
        std::fprintf(stderr, "uvs_host_check_and_shift: %s\n", e.what());
        rc = UVS_ERR_HIP;
    }
    uvs_tri_destroy(tri);
    return rc;
}

// Estimator::setDeviceTriangulation: off by default, a handle while on, none after it is switched off again.  Returns the three observations as bits 0 .. 2.
extern "C" int uvs_host_device_triangulation_switch() {
    try {
        setEurocParameters();
        Estimator est;
        int bits = (est.tri == nullptr && est.f_manager.tri == nullptr) ? 1 : 0;
        est.setDeviceTriangulation(true);
        bits |= (est.tri != nullptr && est.f_manager.tri == est.tri) ? 2 : 0;
        est.setDeviceTriangulation(false);
        bits |= (est.tri == nullptr && est.f_manager.tri == nullptr) ? 4 : 0;
        return bits;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "uvs_host_device_triangulation_switch: %s\n", e.what());
        return -1;
    }
}
