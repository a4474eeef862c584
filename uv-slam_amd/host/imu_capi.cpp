// imu_capi.cpp -- test hooks for the pre-integration of the host mirror (integration_base.h) and its device route (Estimator::setDeviceIntegration).
// Apart from host_capi.cpp because that file is also compiled into the oracle-backed library (oracle/Makefile), and the CPU oracle has no uvs_imu_*.
//   uvs_host_imu_integrate        IntegrationBase driven over a sample list by push_back, optionally followed by repropagate -> its block.  Host code
//                                 only: no GPU is needed.
//   uvs_host_imu_segment          a frame sequence (the file of uvs_host_replay_sequence) through an Estimator with the device route on or off ->
//                                 the blocks of pre_integrations[1 .. WINDOW_SIZE] after the last image, and the samples each of them was made from.
//   uvs_host_device_integration_switch   Estimator::setDeviceIntegration makes and frees the handle.
#include <cstdio>
#include <cstring>
#include "estimator.h"

namespace {

void block_of(const IntegrationBase& pre, int frame_i, uvs_imu_block* out) {
    std::memset(out, 0, sizeof(*out));
    out->sum_dt = pre.sum_dt;
    for (int a = 0; a < 3; ++a) {
        out->delta_p[a] = pre.delta_p(a); out->delta_v[a] = pre.delta_v(a);
        out->linearized_ba[a] = pre.linearized_ba(a); out->linearized_bg[a] = pre.linearized_bg(a);
    }
    out->delta_q[0] = pre.delta_q.x(); out->delta_q[1] = pre.delta_q.y(); out->delta_q[2] = pre.delta_q.z(); out->delta_q[3] = pre.delta_q.w();
    std::memcpy(out->jacobian, pre.jacobian, sizeof(out->jacobian)); std::memcpy(out->covariance, pre.covariance, sizeof(out->covariance));
    out->frame_i = frame_i; out->skip = pre.sum_dt > 10.0 ? 1 : 0;
}

Eigen::Vector3d vec3(const double* v) { return Eigen::Vector3d(v[0], v[1], v[2]); }

}  // namespace

// acc_0 / gyr_0 / ba / bg [3]; dt [n], acc / gyr [n][3]; re_ba / re_bg: both null, or the biases of a repropagate() after the samples
extern "C" int uvs_host_imu_integrate(int n, const double* acc_0, const double* gyr_0, const double* ba, const double* bg, const double* dt,
                                      const double* acc, const double* gyr, const double* re_ba, const double* re_bg, uvs_imu_block* out) {
    if (n < 0 || !acc_0 || !gyr_0 || !ba || !bg || !out || (n > 0 && (!dt || !acc || !gyr)) || (re_ba == nullptr) != (re_bg == nullptr)) return -1;
    setEurocParameters();
    IntegrationBase pre(vec3(acc_0), vec3(gyr_0), vec3(ba), vec3(bg));
    for (int k = 0; k < n; ++k) pre.push_back(dt[k], vec3(acc + 3 * k), vec3(gyr + 3 * k));
    if (re_ba) pre.repropagate(vec3(re_ba), vec3(re_bg));
    block_of(pre, 0, out);
    return 0;
}

// The sequence file of uvs_host_replay_sequence (host_capi.cpp), its first n_images frames.  blocks[WINDOW_SIZE] = pre_integrations[1 .. WINDOW_SIZE]
// after the last image; start[WINDOW_SIZE][6] = their linearized_acc, linearized_gyr; n_samples[WINDOW_SIZE]; samples[WINDOW_SIZE][cap][7] =
// (dt, acc, gyr) of the slot's recorded samples; flags[n_images] = the marginalization flag of each image processed after initialization, else -1.
// Returns 0, or < 0: -1 file, -2 format, -4 not initialised, -6 a slot holds more than cap samples, -10 an exception (its text on stderr).
extern "C" int uvs_host_imu_segment(const char* in_path, int n_images, int use_device, uvs_imu_block* blocks, double* start, int* n_samples,
                                    double* samples, int cap, int* flags) {
    FILE* f = std::fopen(in_path, "rb");
    if (!f) return -1;
    std::vector<double> d;
    { std::fseek(f, 0, SEEK_END); const long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET); d.resize(sz / 8); const bool ok = std::fread(d.data(), 8, d.size(), f) == d.size(); std::fclose(f); if (!ok) return -1; }
    size_t p = 0;
    auto next = [&]() -> double { return p < d.size() ? d[p++] : 0.0; };
    if (next() != (double)0x55565351 || d.size() < 2 + 11 * 16) return -2;
    const int n_frames = (int)next();
    if (n_images > n_frames) return -2;
    const double* pose0 = d.data() + p; p += 77;
    const double* sb0 = d.data() + p; p += 99;
    setEurocParameters();
    try {
        Estimator est;
        est.clearState();
        est.setParameter();
        est.setDeviceIntegration(use_device != 0);
        est.setInitialWindow((const double (*)[7])pose0, (const double (*)[9])sb0);
        for (int fr = 0; fr < n_images; ++fr) {
            std_msgs::Header header; header.stamp.t = next();
            const int n_imu = (int)next();
            for (int k = 0; k < n_imu; ++k) {
                double v[7];
                for (double& x : v) x = next();
                est.processIMU(v[0], vec3(v + 1), vec3(v + 4));
            }
            FeatureManager::ImagePoints image; FeatureManager::ImageLines image_line;
            const int n_pts = (int)next();
            for (int k = 0; k < n_pts; ++k) {
                const int id = (int)next(); Eigen::Matrix<double, 7, 1> m;
                for (int q = 0; q < 7; ++q) m(q) = next();
                image[id].emplace_back(0, m);
            }
            const int n_lines = (int)next();
            for (int k = 0; k < n_lines; ++k) {
                const int id = (int)next(); Eigen::Matrix<double, 15, 1> m;
                for (int q = 0; q < 15; ++q) m(q) = next();
                image_line[id].push_back(m);
            }
            if (p > d.size()) return -2;
            const bool filling = est.solver_flag == Estimator::INITIAL && est.frame_count < WINDOW_SIZE;
            est.processImage(image, image_line, header);
            flags[fr] = filling ? -1 : (int)est.marginalization_flag;
            if (!filling && est.solver_flag == Estimator::INITIAL) return -4;
        }
        est.finishMarginalization();
        if (use_device && est.imu == nullptr) return -7;
        for (int i = 1; i <= WINDOW_SIZE; ++i) {
            const IntegrationBase* pre = est.pre_integrations[i];
            if (!pre) return -4;
            block_of(*pre, i - 1, blocks + (i - 1));
            for (int a = 0; a < 3; ++a) { start[6 * (i - 1) + a] = pre->linearized_acc(a); start[6 * (i - 1) + 3 + a] = pre->linearized_gyr(a); }
            const int m = (int)est.dt_buf[i].size();
            if (m > cap) return -6;
            n_samples[i - 1] = m;
            for (int k = 0; k < m; ++k) {
                double* row = samples + ((size_t)(i - 1) * cap + k) * 7;
                row[0] = est.dt_buf[i][k];
                for (int a = 0; a < 3; ++a) { row[1 + a] = est.linear_acceleration_buf[i][k](a); row[4 + a] = est.angular_velocity_buf[i][k](a); }
            }
        }
    } catch (const std::exception& e) { std::fprintf(stderr, "uvs_host_imu_segment: %s\n", e.what()); return -10; }
    return 0;
}

// Estimator::setDeviceIntegration: off by default, a handle while on, none after it is switched off again.  Returns the three observations as bits 0 .. 2.
extern "C" int uvs_host_device_integration_switch() {
    try {
        setEurocParameters();
        Estimator est;
        int bits = est.imu == nullptr ? 1 : 0;
        est.setDeviceIntegration(true);
        bits |= est.imu != nullptr ? 2 : 0;
        est.setDeviceIntegration(false);
        bits |= est.imu == nullptr ? 4 : 0;
        return bits;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "uvs_host_device_integration_switch: %s\n", e.what());
        return -1;
    }
}
