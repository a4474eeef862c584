// relative_pose_capi.cpp -- test hooks for the bootstrap's choice of its reference frame in the host mirror (FeatureManager::getCorresponding,
// Estimator::relativePose).  Apart from host_capi.cpp because that file is also compiled into the oracle-backed library (oracle/Makefile), and the
// CPU oracle has no uvs_rp_*.
//   uvs_host_get_corresponding   FeatureManager::getCorresponding on hand-made tracks.  Host code only: no GPU is needed.
//   uvs_host_relative_pose       the same tracks through Estimator::relativePose (ONE uvs_rp_relative_pose call for the ten pairs of the window).
// Tracks: start[n_tracks], n_views[n_tracks], pts[sum of n_views][3] = the normalised points (x, y, 1), track after track, view after view.
#include <cstdio>
#include "estimator.h"

namespace {

void fill_tracks(FeatureManager& fm, int n_tracks, const int* start, const int* n_views, const double* pts) {
    size_t at = 0;
    for (int k = 0; k < n_tracks; ++k) {
        FeaturePerId f(k, start[k]);
        for (int v = 0; v < n_views[k]; ++v, ++at) f.feature_per_frame.emplace_back(Eigen::Vector3d(pts[3 * at], pts[3 * at + 1], pts[3 * at + 2]));
        fm.feature.push_back(f);
    }
}

}  // namespace

// left / right [capacity][3].  Returns the number of correspondences (the first `capacity` of them are written), or -1.
extern "C" int uvs_host_get_corresponding(int n_tracks, const int* start, const int* n_views, const double* pts, int frame_l, int frame_r,
                                          double* left, double* right, int capacity) {
    if (n_tracks < 0 || (n_tracks > 0 && (!start || !n_views || !pts)) || !left || !right || capacity < 0) return -1;
    Eigen::Matrix3d Rs[WINDOW_SIZE + 1];
    FeatureManager fm(Rs);
    fill_tracks(fm, n_tracks, start, n_views, pts);
    const auto corres = fm.getCorresponding(frame_l, frame_r);
    for (int i = 0; i < (int)corres.size() && i < capacity; ++i)
        for (int a = 0; a < 3; ++a) { left[3 * i + a] = corres[i].first(a); right[3 * i + a] = corres[i].second(a); }
    return (int)corres.size();
}

// relative_R[9] (row-major), relative_T[3], l.  Returns 1 (found), 0 (no pair of the window passed; the outputs are untouched), or -10: an
// exception (its text on stderr).
extern "C" int uvs_host_relative_pose(int n_tracks, const int* start, const int* n_views, const double* pts, unsigned long long seed,
                                      double* relative_R, double* relative_T, int* l) {
    if (n_tracks < 0 || (n_tracks > 0 && (!start || !n_views || !pts)) || !relative_R || !relative_T || !l) return -1;
    setEurocParameters();
    try {
        Estimator est;
        est.clearState();
        est.setParameter();
        fill_tracks(est.f_manager, n_tracks, start, n_views, pts);
        est.rp_seed = seed;
        Eigen::Matrix3d R; Eigen::Vector3d T; int ll = -1;
        if (!est.relativePose(R, T, ll)) return 0;
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) relative_R[3 * r + c] = R(r, c);
            relative_T[r] = T(r);
        }
        *l = ll;
        return 1;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "uvs_host_relative_pose: %s\n", e.what());
        return -10;
    }
}
