// uvs_camera_models.h -- the three camera models of the front ends in FP64, one statement for the device and the host: the radial-tangential
// pinhole (reference camera_models/PinholeCamera.cc:450-510 liftProjective, 678-694 distortion), MEI (CataCamera.cc:556-659 liftProjective /
// spaceToPlane, :766-782 distortion) and Kannala-Brandt (EquidistantCamera.cc:428-461, backprojectSymmetric :716-818).  lift: pixel -> ray and
// normalized point; project: ray -> pixel; the check and the packing of a uvs_camera_model (with the Kannala-Brandt th_max search) and of a
// uvs_kf_camera on the host.  include/uvs_solver.h states the operation order; IEEE multiplies, adds, divides and square roots in that order:
// the units that include this are compiled with -ffp-contract=off, and tests/cm_ref.py and tests/kf_ref.py (lift) restate it.  Shared by
// csrc/uvs_camera_models.hip (uvs_ft_lift, uvs_ft_project), csrc/uvs_line_undistort.hip (the map), the three units that lift in a kernel
// (uvs_feature_track, uvs_feature_detect, uvs_keyframe_features) and the host mirror.
#pragma once
#include <cmath>
#include <string>

#include "../../include/uvs_solver.h"

#if defined(__HIPCC__)
#define UVS_LIFT_HD __host__ __device__ __forceinline__
#else
#define UVS_LIFT_HD inline
#endif

// The camera as every kernel takes it, 120 bytes, by value as a kernel argument: wave-uniform, so the branch on the model id is a scalar
// branch.  It is the handle's model where one is set, else the call's uvs_kf_camera packed as a PINHOLE.  model < 0 on the host: the handle
// holds no model.
//   PINHOLE          (sx, sy, u0, v0) = (fx, fy, cx, cy), c = k1 k2 p1 p2 -,      flag: some coefficient is not 0
//   MEI              (sx, sy, u0, v0) = (gamma1, gamma2, u0, v0), c = k1 k2 p1 p2 xi, flag: some coefficient is not 0 (!m_noDistortion)
//   KANNALA_BRANDT   (sx, sy, u0, v0) = (mu, mv, u0, v0), c = k2 k3 k4 k5 th_max, flag: some k is not 0; r_max = r(th_max)
struct UvsCamDev {
    int model, flag;
    double inv_K11, inv_K13, inv_K22, inv_K23;
    double sx, sy, u0, v0;
    double c[5];
    double r_max;
};

inline UvsCamDev uvs_cam_none() { UvsCamDev m = {}; m.model = -1; return m; }

// ---- Kannala-Brandt: r(th), r'(th) and the root of r(th) = rr on the first monotone branch
UVS_LIFT_HD double uvs_kb_r(const UvsCamDev& m, double th) {
    const double t = th * th;
    return th + th * (t * (m.c[0] + t * (m.c[1] + t * (m.c[2] + t * m.c[3]))));
}
UVS_LIFT_HD double uvs_kb_dr(const UvsCamDev& m, double th) {
    const double t = th * th;
    return 1.0 + t * (3.0 * m.c[0] + t * (5.0 * m.c[1] + t * (7.0 * m.c[2] + t * (9.0 * m.c[3]))));
}
// A fixed bound of steps, each one evaluation of r and r' and one divide; the only data-dependent exits are the `break`s (2 .. 7 steps, 3.3 to
// 3.8 on average, over every pixel of the images of the three shipped Kannala-Brandt configurations)
UVS_LIFT_HD double uvs_kb_theta(const UvsCamDev& m, double rr) {
    if (!m.flag || !(rr < m.r_max)) return rr;
    double lo = 0.0, hi = m.c[4], th = rr < hi ? rr : hi, prev = th;
    for (int it = 0; it < UVS_CAM_KB_ITERATIONS; ++it) {
        const double f = uvs_kb_r(m, th) - rr;
        if (f == 0.0) break;
        if (f > 0.0) hi = th; else lo = th;
        double tn = th - f / uvs_kb_dr(m, th);
        if (tn == th || tn == prev) break;                    // the step no longer moves, or steps back: two neighbouring doubles straddle the root
        if (!(tn >= lo && tn <= hi)) tn = 0.5 * (lo + hi);
        prev = th; th = tn;
    }
    return th;
}

// ---- lift: pixel (x, y) -> ray[3] and the normalized point (ray[0] / ray[2], ray[1] / ray[2])
UVS_LIFT_HD void uvs_cam_lift(const UvsCamDev& m, double x, double y, double* ray, double& nx, double& ny) {
    if (m.model == UVS_CAM_KANNALA_BRANDT) {
        const double px = m.inv_K11 * x + m.inv_K13, py = m.inv_K22 * y + m.inv_K23;
        const double rr = sqrt(px * px + py * py);
        const double th = uvs_kb_theta(m, rr);
        const double s = sin(th), c = cos(th);
        if (rr < 1e-10) { ray[0] = s; ray[1] = 0.0; } else { ray[0] = (s * px) / rr; ray[1] = (s * py) / rr; }
        ray[2] = c;
    } else {                                                  // PINHOLE and MEI: the recursive distortion model
        const double mx_d = m.inv_K11 * x + m.inv_K13, my_d = m.inv_K22 * y + m.inv_K23;
        double mx = mx_d, my = my_d;
        if (m.flag) {                                         // distortion() at (mx_d, my_d), then 7 times at the running estimate
            const double k1 = m.c[0], k2 = m.c[1], p1 = m.c[2], p2 = m.c[3];
            for (int it = 0; it < 8; ++it) {
                const double mx2 = mx * mx, my2 = my * my, mxy = mx * my, rho2 = mx2 + my2;
                const double rad = k1 * rho2 + k2 * rho2 * rho2;
                const double dx = mx * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2);
                const double dy = my * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2);
                mx = mx_d - dx; my = my_d - dy;
            }
        }
        ray[0] = mx; ray[1] = my;
        if (m.model == UVS_CAM_PINHOLE) { ray[2] = 1.0; nx = mx; ny = my; return; }
        const double xi = m.c[4];
        if (xi == 1.0) ray[2] = ((1.0 - mx * mx) - my * my) / 2.0;
        else {
            const double rho2 = mx * mx + my * my;
            ray[2] = 1.0 - (xi * (rho2 + 1.0)) / (xi + sqrt(1.0 + (1.0 - xi * xi) * rho2));
        }
    }
    nx = ray[0] / ray[2]; ny = ray[1] / ray[2];
}

// ---- project: ray (X, Y, Z) -> pixel (spaceToPlane)
UVS_LIFT_HD void uvs_cam_project(const UvsCamDev& m, double X, double Y, double Z, double& u, double& v) {
    if (m.model == UVS_CAM_KANNALA_BRANDT) {
        const double h = sqrt(X * X + Y * Y);
        const double q = uvs_kb_r(m, atan2(h, Z));
        double ux = q, uy = 0.0;
        if (h != 0.0) { ux = (q * X) / h; uy = (q * Y) / h; }
        u = m.sx * ux + m.u0; v = m.sy * uy + m.v0;
    } else if (m.model == UVS_CAM_MEI) {
        const double z = Z + m.c[4] * sqrt(X * X + (Y * Y + Z * Z));
        double x = X / z, y = Y / z;
        if (m.flag) {
            const double x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
            const double rad = m.c[0] * r2 + m.c[1] * r2 * r2;
            const double dx = x * rad + 2.0 * m.c[2] * xy + m.c[3] * (r2 + 2.0 * x2);
            const double dy = y * rad + 2.0 * m.c[3] * xy + m.c[2] * (r2 + 2.0 * y2);
            x = x + dx; y = y + dy;
        }
        u = m.sx * x + m.u0; v = m.sy * y + m.v0;
    } else {                                                  // the forward map of uvs_lt_set_undistort
        const double x = X / Z, y = Y / Z;
        const double x2 = x * x, y2 = y * y, xy = x * y, r2 = x2 + y2;
        const double kr = 1.0 + (m.c[0] * r2 + m.c[1] * (r2 * r2));
        const double xd = x * kr + ((2.0 * m.c[2]) * xy + m.c[3] * (r2 + 2.0 * x2));
        const double yd = y * kr + (m.c[2] * (r2 + 2.0 * y2) + (2.0 * m.c[3]) * xy);
        u = m.sx * xd + m.u0; v = m.sy * yd + m.v0;
    }
}

// ---- host: the check of a uvs_camera_model and its packing; `fn` prefixes the error text
inline int uvs_cam_param_count(int model) { return model == UVS_CAM_PINHOLE ? 8 : model == UVS_CAM_MEI ? 9 : model == UVS_CAM_KANNALA_BRANDT ? 8 : 0; }

// `kf`: the model is a call's uvs_kf_camera (uvs_cam_pinhole), whose two texts are older than the models'
inline int uvs_cam_check(const uvs_camera_model* model, const std::string& fn, std::string& err, bool kf = false) {
    const int n = uvs_cam_param_count(model->model);
    if (!n) { err = fn + ": unknown camera model"; return UVS_ERR_INVALID_ARG; }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(model->p[i])) { err = fn + (kf ? ": the camera must be finite" : ": the camera model must be finite"); return UVS_ERR_INVALID_ARG; }
    const double* p = model->p;
    const double sx = model->model == UVS_CAM_PINHOLE ? p[0] : model->model == UVS_CAM_MEI ? p[5] : p[4];
    const double sy = model->model == UVS_CAM_PINHOLE ? p[1] : model->model == UVS_CAM_MEI ? p[6] : p[5];
    if (!(sx > 0.0) || !(sy > 0.0)) {
        err = fn + (kf ? ": fx and fy must be positive" : ": the camera model's scales (fx fy, gamma1 gamma2, mu mv) must be positive"); return UVS_ERR_INVALID_ARG;
    }
    if (model->model == UVS_CAM_MEI && p[0] < 0.0) { err = fn + ": xi must not be negative"; return UVS_ERR_INVALID_ARG; }
    return UVS_OK;
}

// th_max of a packed Kannala-Brandt model (c[0 .. 3] set): the first th in (0, pi] with r'(th) <= 0, as the lower of the two neighbouring
// doubles the bisection ends at, or pi
inline double uvs_kb_theta_max(const UvsCamDev& m) {
    const double pi = 3.141592653589793, step = pi / 4096.0;
    for (int i = 1; i <= 4096; ++i) {
        if (uvs_kb_dr(m, (double)i * step) > 0.0) continue;
        double lo = (double)(i - 1) * step, hi = (double)i * step;
        for (;;) {
            const double mid = 0.5 * (lo + hi);
            if (mid == lo || mid == hi) return lo;
            if (uvs_kb_dr(m, mid) > 0.0) lo = mid; else hi = mid;
        }
    }
    return pi;
}

// a checked model -> what the kernels take
inline UvsCamDev uvs_cam_pack(const uvs_camera_model& model) {
    const double* p = model.p;
    UvsCamDev m = {};
    m.model = model.model;
    if (model.model == UVS_CAM_PINHOLE) { m.sx = p[0]; m.sy = p[1]; m.u0 = p[2]; m.v0 = p[3]; for (int i = 0; i < 4; ++i) m.c[i] = p[4 + i]; }
    else if (model.model == UVS_CAM_MEI) { m.sx = p[5]; m.sy = p[6]; m.u0 = p[7]; m.v0 = p[8]; for (int i = 0; i < 4; ++i) m.c[i] = p[1 + i]; m.c[4] = p[0]; }
    else { m.sx = p[4]; m.sy = p[5]; m.u0 = p[6]; m.v0 = p[7]; for (int i = 0; i < 4; ++i) m.c[i] = p[i]; }
    m.flag = !(m.c[0] == 0.0 && m.c[1] == 0.0 && m.c[2] == 0.0 && m.c[3] == 0.0);
    m.inv_K11 = 1.0 / m.sx; m.inv_K13 = -m.u0 / m.sx; m.inv_K22 = 1.0 / m.sy; m.inv_K23 = -m.v0 / m.sy;
    if (model.model == UVS_CAM_KANNALA_BRANDT) { m.c[4] = uvs_kb_theta_max(m); m.r_max = uvs_kb_r(m, m.c[4]); }
    return m;
}

// the model argument of a set call or a batch call: checked and packed into `out`
inline int uvs_cam_take(const uvs_camera_model* model, const std::string& fn, std::string& err, UvsCamDev* out, bool kf = false) {
    if (const int rc = uvs_cam_check(model, fn, err, kf)) return rc;
    *out = uvs_cam_pack(*model);
    return UVS_OK;
}

// a uvs_kf_camera is p[0 .. 8) of a PINHOLE model
inline uvs_camera_model uvs_cam_pinhole(const uvs_kf_camera& c) {
    uvs_camera_model m = {};
    m.model = UVS_CAM_PINHOLE;
    m.p[0] = c.fx; m.p[1] = c.fy; m.p[2] = c.cx; m.p[3] = c.cy; m.p[4] = c.k1; m.p[5] = c.k2; m.p[6] = c.p1; m.p[7] = c.p2;
    return m;
}

// the camera of a call that lifts: the handle's model where it holds one (`camera` is not looked at), else the call's camera, checked
inline int uvs_cam_of_call(const UvsCamDev& held, const uvs_kf_camera* camera, const std::string& fn, std::string& err, UvsCamDev* out) {
    if (held.model >= 0) { *out = held; return UVS_OK; }
    const uvs_camera_model m = uvs_cam_pinhole(*camera);
    return uvs_cam_take(&m, fn, err, out, true);
}
