"""The camera models of the front ends (include/uvs_solver.h: uvs_camera_model; csrc/uvs_camera_models.h), twice:

  * the FP64 numpy restatement in the header's operation order (pack, lift, project, build_map), one rounding per operation (numpy evaluates an
    expression operation by operation, never fused).  PINHOLE and MEI use multiplies, adds, divides and sqrt only, so the device equals it bit
    for bit; KANNALA_BRANDT also takes sin, cos and atan2 from the platform's library, so it is held to a tolerance;
  * a 60-digit mpmath evaluation of the REFERENCE's definition (lift_hp, project_hp): for Kannala-Brandt ALL roots of the polynomial, the
    smallest non-negative real one (EquidistantCamera::backprojectSymmetric's gates), then sin / cos with phi = atan2.  Where that root lies
    beyond the first monotone branch (or there is none) the library's stated deviation applies, th = r, and lift_hp reports the pixel.

TEST INFRASTRUCTURE ONLY."""
import types

import mpmath
import numpy as np

PINHOLE, MEI, KB = 0, 1, 2
KB_ITERATIONS = 32
LIMIT = 1 << 24
_PI = np.float64(3.141592653589793)
F = np.float64


# ---- the packed model (UvsCamDev)
def _kb_r(c, th):
    t = th * th
    return th + th * (t * (c[0] + t * (c[1] + t * (c[2] + t * c[3]))))


def _kb_dr(c, th):
    t = th * th
    return F(1.0) + t * (F(3.0) * c[0] + t * (F(5.0) * c[1] + t * (F(7.0) * c[2] + t * (F(9.0) * c[3]))))


def kb_theta_max(c):
    """The first th in (0, pi] with r'(th) <= 0 as the lower of the neighbouring doubles the bisection ends at, or pi."""
    step = _PI / F(4096.0)
    for i in range(1, 4097):
        if _kb_dr(c, F(i) * step) > 0.0:
            continue
        lo, hi = F(i - 1) * step, F(i) * step
        while True:
            mid = F(0.5) * (lo + hi)
            if mid == lo or mid == hi:
                return lo
            if _kb_dr(c, mid) > 0.0:
                lo = mid
            else:
                hi = mid
    return _PI


def pack(model, params):
    p = [F(v) for v in params]
    P = types.SimpleNamespace(model=int(model), r_max=F(0.0))
    if model == PINHOLE:
        P.sx, P.sy, P.u0, P.v0 = p[0:4]; P.c = p[4:8] + [F(0.0)]
    elif model == MEI:
        P.sx, P.sy, P.u0, P.v0 = p[5:9]; P.c = p[1:5] + [p[0]]
    elif model == KB:
        P.sx, P.sy, P.u0, P.v0 = p[4:8]; P.c = p[0:4] + [F(0.0)]
    else:
        raise ValueError("unknown model")
    P.flag = any(v != 0.0 for v in P.c[:4])
    P.inv_K11 = F(1.0) / P.sx; P.inv_K13 = -P.u0 / P.sx; P.inv_K22 = F(1.0) / P.sy; P.inv_K23 = -P.v0 / P.sy
    if model == KB:
        P.c[4] = kb_theta_max(P.c); P.r_max = _kb_r(P.c, P.c[4])
    return P


def kb_theta(P, rr, return_steps=False):
    """The root search of uvs_kb_theta for an array of rr -> th (and the steps each element took)."""
    rr = np.asarray(rr, F)
    out = rr.copy()
    steps = np.zeros(rr.shape, np.int32)
    with np.errstate(all="ignore"):
        act = np.flatnonzero((rr < P.r_max) & P.flag)
        r = rr[act]
        lo = np.zeros_like(r); hi = np.full_like(r, P.c[4])
        th = np.where(r < hi, r, hi); prev = th
        done = np.zeros(r.shape, bool); n = np.zeros(r.shape, np.int32)
        for _ in range(KB_ITERATIONS):
            if done.all():
                break
            f = _kb_r(P.c, th) - r
            live = ~done & ~(f == 0.0)
            hi = np.where(live & (f > 0.0), th, hi); lo = np.where(live & ~(f > 0.0), th, lo)
            tn = th - f / _kb_dr(P.c, th)
            move = live & ~(tn == th) & ~(tn == prev)
            tn = np.where((tn >= lo) & (tn <= hi), tn, F(0.5) * (lo + hi))
            prev = np.where(move, th, prev); th = np.where(move, tn, th)
            n += ~done
            done |= ~move
        out[act] = th; steps[act] = n
    return (out, steps) if return_steps else out


def _distortion(c, x, y):
    x2 = x * x; y2 = y * y; xy = x * y; r2 = x2 + y2
    rad = c[0] * r2 + c[1] * r2 * r2
    return x * rad + F(2.0) * c[2] * xy + c[3] * (r2 + F(2.0) * x2), y * rad + F(2.0) * c[3] * xy + c[2] * (r2 + F(2.0) * y2)


def lift(model, params, xy):
    """xy [n, 2] pixels -> (ray [n, 3], norm [n, 2])."""
    P = pack(model, params)
    xy = np.asarray(xy, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        xd = P.inv_K11 * xy[:, 0] + P.inv_K13; yd = P.inv_K22 * xy[:, 1] + P.inv_K23
        if model == KB:
            rr = np.sqrt(xd * xd + yd * yd)
            th = kb_theta(P, rr)
            s = np.sin(th); c = np.cos(th)
            tiny = rr < 1e-10
            X = np.where(tiny, s, (s * xd) / rr); Y = np.where(tiny, F(0.0), (s * yd) / rr); Z = c
        else:
            xu, yu = xd, yd
            if P.flag:
                for _ in range(8):
                    dx, dy = _distortion(P.c, xu, yu)
                    xu = xd - dx; yu = yd - dy
            X, Y = xu, yu
            if model == PINHOLE:
                return np.stack([X, Y, np.ones_like(X)], 1), np.stack([X, Y], 1)
            xi = P.c[4]
            if xi == 1.0:
                Z = ((F(1.0) - xu * xu) - yu * yu) / F(2.0)
            else:
                rho2 = xu * xu + yu * yu
                Z = F(1.0) - (xi * (rho2 + F(1.0))) / (xi + np.sqrt(F(1.0) + (F(1.0) - xi * xi) * rho2))
        return np.stack([X, Y, Z], 1), np.stack([X / Z, Y / Z], 1)


def _project(P, X, Y, Z):
    with np.errstate(all="ignore"):
        if P.model == KB:
            h = np.sqrt(X * X + Y * Y)
            q = _kb_r(P.c, np.arctan2(h, Z))
            zero = h == 0.0
            ux = np.where(zero, q, (q * X) / h); uy = np.where(zero, F(0.0), (q * Y) / h)
            return P.sx * ux + P.u0, P.sy * uy + P.v0
        if P.model == MEI:
            z = Z + P.c[4] * np.sqrt(X * X + (Y * Y + Z * Z))
            x = X / z; y = Y / z
            if P.flag:
                dx, dy = _distortion(P.c, x, y)
                x = x + dx; y = y + dy
            return P.sx * x + P.u0, P.sy * y + P.v0
        x = X / Z; y = Y / Z
        x2 = x * x; y2 = y * y; xy = x * y; r2 = x2 + y2
        kr = F(1.0) + (P.c[0] * r2 + P.c[1] * (r2 * r2))
        xd = x * kr + ((F(2.0) * P.c[2]) * xy + P.c[3] * (r2 + F(2.0) * x2))
        yd = y * kr + (P.c[2] * (r2 + F(2.0) * y2) + (F(2.0) * P.c[3]) * xy)
        return P.sx * xd + P.u0, P.sy * yd + P.v0


def project(model, params, ray):
    """ray [n, 3] -> xy [n, 2] pixels."""
    ray = np.asarray(ray, F).reshape(-1, 3)
    u, v = _project(pack(model, params), ray[:, 0], ray[:, 1], ray[:, 2])
    return np.stack([u, v], 1)


def _fix(m):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(F(32.0) * np.asarray(m, F))
        v = np.where(np.isfinite(v), np.clip(v, -float(LIMIT), float(LIMIT)), -float(LIMIT))
    return v.astype(np.int32)


def build_map(model, params, W, H, out_cam, cm=0, rm=0, slack=None):
    """The map of uvs_lt_set_undistort_model [Ho, Wo, 2] int32.  With `slack` (pixels of the raw image) also the mask [Ho, Wo, 2] of the words
    whose value before rounding, 32 m, lies within 32 slack of a half-integer: the words another correctly working sin / cos / atan2 may round
    the other way."""
    fx, fy, cx, cy = [F(v) for v in out_cam]
    Wo, Ho = W - 2 * cm, H - 2 * rm
    vo, uo = np.mgrid[0:Ho, 0:Wo]
    u = (uo + cm).astype(F); v = (vo + rm).astype(F)
    x = (u - cx) / fx; y = (v - cy) / fy
    mx, my = _project(pack(model, params), x.ravel(), y.ravel(), np.ones(x.size))
    m = np.stack([mx.reshape(Ho, Wo), my.reshape(Ho, Wo)], -1)
    words = _fix(m)
    if slack is None:
        return words
    with np.errstate(invalid="ignore"):
        s = F(32.0) * m
        near = np.abs(s - np.floor(s) - 0.5) <= 32.0 * slack
    return words, near


# ---- 60 digits: the reference's definition
mpmath.mp.dps = 60
_TOL = mpmath.mpf("1e-10")


def _mp_params(params):
    return [mpmath.mpf(float(v)) for v in params]


def kb_root_hp(k, r):
    """backprojectSymmetric's th for mpf r: the smallest non-negative real root among ALL roots of the polynomial (the reference's degree rule:
    the power drops by 2 for every zero coefficient; its gates |imag| <= 1e-10, real >= -1e-10, a negative real clamped to 0), or None."""
    npow = 9 - 2 * sum(1 for v in k if v == 0)
    if npow == 1:
        return r
    coeffs = [mpmath.mpf(0)] * (npow + 1)
    coeffs[0] = -r; coeffs[1] = mpmath.mpf(1)
    for i, p in enumerate((3, 5, 7, 9)):
        if npow >= p:
            coeffs[p] = k[i]
    roots = mpmath.polyroots(coeffs[::-1], maxsteps=500, extraprec=400)
    ths = [max(z.real, mpmath.mpf(0)) for z in roots if abs(z.imag) <= _TOL and z.real >= -_TOL]
    return min(ths) if ths else None


def lift_hp(model, params, xy):
    """-> (ray [n, 3] of mpf, deviates [n] bool): the reference's liftProjective at 60 digits.  deviates: a Kannala-Brandt pixel whose reference
    root is beyond th_max (a later branch) or missing, where the ray is the library's th = r."""
    p = _mp_params(params)
    P = pack(model, params)
    rays, dev = [], []
    for x, y in np.asarray(xy, F).reshape(-1, 2):
        x = mpmath.mpf(float(x)); y = mpmath.mpf(float(y))
        if model == KB:
            k = p[0:4]; mu, mv, u0, v0 = p[4:8]
            px = (x - u0) / mu; py = (y - v0) / mv
            r = mpmath.sqrt(px * px + py * py)
            th = kb_root_hp(k, r)
            d = th is None or th > mpmath.mpf(float(P.c[4])) * (1 + mpmath.mpf("1e-12"))
            if d:
                th = r
            phi = mpmath.mpf(0) if r < _TOL else mpmath.atan2(py, px)
            rays.append([mpmath.sin(th) * mpmath.cos(phi), mpmath.sin(th) * mpmath.sin(phi), mpmath.cos(th)]); dev.append(d)
            continue
        if model == PINHOLE:
            fx, fy, cx, cy = p[0:4]; c = p[4:8]
        else:
            xi = p[0]; c = p[1:5]; fx, fy, cx, cy = p[5:9]
        xd = (x - cx) / fx; yd = (y - cy) / fy
        xu, yu = xd, yd
        if any(v != 0 for v in c):
            for _ in range(8):                               # the reference's recursive model IS its definition: eight passes, not the limit
                x2 = xu * xu; y2 = yu * yu; xy_ = xu * yu; r2 = x2 + y2
                rad = c[0] * r2 + c[1] * r2 * r2
                dx = xu * rad + 2 * c[2] * xy_ + c[3] * (r2 + 2 * x2); dy = yu * rad + 2 * c[3] * xy_ + c[2] * (r2 + 2 * y2)
                xu = xd - dx; yu = yd - dy
        if model == PINHOLE:
            z = mpmath.mpf(1)
        elif xi == 1:
            z = (1 - xu * xu - yu * yu) / 2
        else:
            rho2 = xu * xu + yu * yu
            z = 1 - xi * (rho2 + 1) / (xi + mpmath.sqrt(1 + (1 - xi * xi) * rho2))
        rays.append([xu, yu, z]); dev.append(False)
    return rays, np.array(dev, bool)


def project_hp(model, params, ray):
    """The reference's spaceToPlane at 60 digits; ray: rows of three mpf (or floats) -> [[u, v]] of mpf."""
    p = _mp_params(params)
    out = []
    for X, Y, Z in ray:
        X, Y, Z = mpmath.mpf(X), mpmath.mpf(Y), mpmath.mpf(Z)
        if model == KB:
            k = p[0:4]; mu, mv, u0, v0 = p[4:8]
            th = mpmath.acos(Z / mpmath.sqrt(X * X + Y * Y + Z * Z)); phi = mpmath.atan2(Y, X)
            q = th + k[0] * th ** 3 + k[1] * th ** 5 + k[2] * th ** 7 + k[3] * th ** 9
            out.append([mu * q * mpmath.cos(phi) + u0, mv * q * mpmath.sin(phi) + v0])
            continue
        if model == PINHOLE:
            fx, fy, cx, cy = p[0:4]; c = p[4:8]; z = Z
        else:
            xi = p[0]; c = p[1:5]; fx, fy, cx, cy = p[5:9]; z = Z + xi * mpmath.sqrt(X * X + Y * Y + Z * Z)
        x = X / z; y = Y / z
        if any(v != 0 for v in c):
            x2 = x * x; y2 = y * y; xy_ = x * y; r2 = x2 + y2
            rad = c[0] * r2 + c[1] * r2 * r2
            x, y = x + x * rad + 2 * c[2] * xy_ + c[3] * (r2 + 2 * x2), y + y * rad + 2 * c[3] * xy_ + c[2] * (r2 + 2 * y2)
        out.append([fx * x + cx, fy * y + cy])
    return out


def ray_error(ray, ray_hp):
    """ray [n, 3] float64 against rows of mpf -> [n] the largest absolute component error, as floats."""
    return np.array([max(abs(float(mpmath.mpf(float(a)) - b)) for a, b in zip(r, h)) for r, h in zip(ray, ray_hp)])
