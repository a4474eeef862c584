// uvs_camera_lift.h -- PinholeCamera::liftProjective (reference camera_models/PinholeCamera.cc:450-510, 678-694) in FP64, shared by the units
// that return normalized image points (uvs_kf_extract's keypoints, uvs_ft_track's tracked points) and by the host mirror, so that there is one
// statement of it.  IEEE multiplies and adds in a fixed order: the units that include it are compiled with -ffp-contract=off, and tests/kf_ref.py
// (lift) restates it.
#pragma once
#include "../../include/uvs_solver.h"

#if defined(__HIPCC__)
#define UVS_LIFT_HD __host__ __device__ __forceinline__
#else
#define UVS_LIFT_HD inline
#endif

// what liftProjective reads of a uvs_kf_camera: the inverse projection (PinholeCamera.cc:292-295) and the distortion coefficients
struct UvsLiftCam { double inv_K11, inv_K13, inv_K22, inv_K23, k1, k2, p1, p2; int distort, pad; };

inline UvsLiftCam uvs_lift_camera(const uvs_kf_camera& c) {
    UvsLiftCam cam;
    cam.inv_K11 = 1.0 / c.fx; cam.inv_K13 = -c.cx / c.fx;
    cam.inv_K22 = 1.0 / c.fy; cam.inv_K23 = -c.cy / c.fy;
    cam.k1 = c.k1; cam.k2 = c.k2; cam.p1 = c.p1; cam.p2 = c.p2;
    cam.distort = !(c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0); cam.pad = 0;
    return cam;
}

// pixel (x, y) -> normalized (mx_u, my_u): the recursive distortion model, distortion() at (mx_d, my_d), then 7 times at the running estimate
UVS_LIFT_HD void uvs_lift_projective(const UvsLiftCam& cam, double x, double y, double& mx_out, double& my_out) {
    const double mx_d = cam.inv_K11 * x + cam.inv_K13, my_d = cam.inv_K22 * y + cam.inv_K23;
    double mx_u = mx_d, my_u = my_d;
    if (cam.distort) {
        for (int it = 0; it < 8; ++it) {
            const double mx2 = mx_u * mx_u, my2 = my_u * my_u, mxy = mx_u * my_u, rho2 = mx2 + my2;
            const double rad = cam.k1 * rho2 + cam.k2 * rho2 * rho2;
            const double dx = mx_u * rad + 2.0 * cam.p1 * mxy + cam.p2 * (rho2 + 2.0 * mx2);
            const double dy = my_u * rad + 2.0 * cam.p2 * mxy + cam.p1 * (rho2 + 2.0 * my2);
            mx_u = mx_d - dx; my_u = my_d - dy;
        }
    }
    mx_out = mx_u; my_out = my_u;
}
