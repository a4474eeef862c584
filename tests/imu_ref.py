"""Reference for the IMU pre-integration (uvs_imu_*, csrc/uvs_imu_preintegrate.hip; the host mirror's IntegrationBase; synth.PreIntegration).

Three statements of IntegrationBase::push_back / propagate / midPointIntegration (integration_base.h:30-158) and of processIMU's dead reckoning
(estimator.cpp:104-117), all on the same FP64 inputs:
  * `preintegrate_hp` / the `*_hp` values: the recursion in 60-digit floating point -- the truth everything else is held to.  It runs on
    decimal.Decimal (precision 60), not on mpmath.mpf: the two are the same arithmetic to the last of the 60 digits that matter here, and the C
    implementation behind Decimal is some twenty times faster, which is what makes the 2 001-sample cases affordable in a test.
    tests/test_imu_ref.py holds it to an mpmath evaluation at 60 digits on a short case.  F and V are walked block-sparse, so an entry that is
    structurally 0 or 1 is exactly that;
  * synth.PreIntegration, the numpy restatement the project ships: its error against the 60-digit values is E_ref (tests/imu_cases.py);
  * `preintegrate_np`: a copy of that restatement with switches for planted defects (without a defect it equals the restatement bit for bit).
The metrics are those the tests assert on (`errors`, `dr_errors`).

TEST INFRASTRUCTURE ONLY."""
import decimal

import numpy as np

from helpers import uvs

synth = uvs.synth
DPS = 60
D = decimal.Decimal
EPS = 2.0 ** -53
NOISE = (synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W)
DEFECTS = ("F012_sign", "v03_half_dt", "noise_slots", "no_normalise", "V66_Rq", "gyr_bias")


# ------------------------------------------------------------------------------------------------ small helpers, any number type
def quat_R(q):
    x, y, z, w = q
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]


def quat_mul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]


def _skew(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _ms(A, s):
    return [[a * s for a in row] for row in A]


def _madd(A, B):
    return [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(A, B)]


def _dvec(v):
    return [D(float(x)) for x in v]


# ------------------------------------------------------------------------------------------------ the 60-digit recursion
def _rows(blocks, ncols):
    """{(row block, column block): 3 x 3 list, or a scalar s for s * I} -> per row a list of (column, value): the structural non-zeros."""
    rows = [[] for _ in range(15)]
    for (rb, cb), M in sorted(blocks.items()):
        for i in range(3):
            if isinstance(M, list):
                rows[3 * rb + i] += [(3 * cb + j, M[i][j]) for j in range(3)]
            else:
                rows[3 * rb + i].append((3 * cb + i, M))
    return rows


def preintegrate_hp(interval, noise=NOISE, state=None, gravity=None, snapshots=()):
    """The recursion at 60 digits -> dict(dp, dq, dv [Decimal], J, C [15][15 Decimal], sum_dt, n; with `state` = (P, R, V): pP, pR, pV).
    `snapshots`: sample counts at which the state is ALSO returned, as result["at"][count] (a long case then yields its prefixes for free)."""
    with decimal.localcontext() as ctx:
        ctx.prec = DPS
        one, half, quarter = D(1), D("0.5"), D("0.25")
        ba, bg = _dvec(interval["ba"]), _dvec(interval["bg"])
        a0, g0 = _dvec(interval["acc_0"]), _dvec(interval["gyr_0"])
        sig = [noise[0], noise[1], noise[0], noise[1], noise[2], noise[3]]
        nz = [D(float(sig[k // 3])) ** 2 for k in range(18)]
        dp, dv, dq, sum_dt = [D(0)] * 3, [D(0)] * 3, [D(0), D(0), D(0), one], D(0)
        J = [[one if i == j else D(0) for j in range(15)] for i in range(15)]
        Cv = [[D(0)] * 15 for _ in range(15)]
        if state is not None:
            wP, wR, wV = _dvec(state[0]), [_dvec(r) for r in np.asarray(state[1], float).reshape(3, 3)], _dvec(state[2])
            grav = _dvec(gravity)
        I3 = [[one, 0, 0], [0, one, 0], [0, 0, one]]
        dts = np.atleast_1d(np.asarray(interval["dt"], float)); accs = np.asarray(interval["acc"], float).reshape(-1, 3); gyrs = np.asarray(interval["gyr"], float).reshape(-1, 3)

        def result(n):
            r = dict(dp=list(dp), dq=list(dq), dv=list(dv), J=[list(r_) for r_ in J], C=[list(r_) for r_ in Cv], sum_dt=sum_dt, n=n)
            if state is not None:
                r.update(pP=list(wP), pR=[list(r_) for r_ in wR], pV=list(wV))
            return r

        at = {}
        if 0 in snapshots:
            at[0] = result(0)
        for n in range(len(dts)):
            dt, a1, g1 = D(float(dts[n])), _dvec(accs[n]), _dvec(gyrs[n])
            a0b = [x - y for x, y in zip(a0, ba)]; a1b = [x - y for x, y in zip(a1, ba)]
            w = [half * (x + y) - z for x, y, z in zip(g0, g1, bg)]
            Rq = quat_R(dq)
            rq = quat_mul(dq, [w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, one])
            Rr = quat_R(rq)
            un = [half * (x + y) for x, y in zip(_mv(Rq, a0b), _mv(Rr, a1b))]
            rp = [p + v * dt + half * u * dt * dt for p, v, u in zip(dp, dv, un)]
            rv = [v + u * dt for v, u in zip(dv, un)]
            Rw, Ra0, Ra1 = _skew(w), _skew(a0b), _skew(a1b)
            T = _madd(I3, _ms(Rw, -dt))
            RrA1 = _mm(Rr, Ra1)
            B1 = _madd(_mm(Rq, Ra0), _mm(RrA1, T)); B3 = _madd(Rq, Rr)
            dt2 = dt * dt
            F = _rows({(0, 0): one, (0, 1): _ms(B1, -quarter * dt2), (0, 2): dt, (0, 3): _ms(B3, -quarter * dt2), (0, 4): _ms(RrA1, quarter * dt2 * dt),
                       (1, 1): T, (1, 4): -dt,
                       (2, 1): _ms(B1, -half * dt), (2, 2): one, (2, 3): _ms(B3, -half * dt), (2, 4): _ms(RrA1, half * dt2),
                       (3, 3): one, (4, 4): one}, 15)
            v03 = _ms(RrA1, -quarter * dt2 * half * dt); v63 = _ms(RrA1, -half * dt * half * dt)
            V = _rows({(0, 0): _ms(Rq, quarter * dt2), (0, 1): v03, (0, 2): _ms(Rr, quarter * dt2), (0, 3): v03,
                       (1, 1): half * dt, (1, 3): half * dt,
                       (2, 0): _ms(Rq, half * dt), (2, 1): v63, (2, 2): _ms(Rr, half * dt), (2, 3): v63,
                       (3, 4): dt, (4, 5): dt}, 18)
            J = [[sum(v * J[k][j] for k, v in F[i]) for j in range(15)] for i in range(15)]
            FC = [[sum(v * Cv[k][j] for k, v in F[i]) for j in range(15)] for i in range(15)]
            Vd = [dict(r) for r in V]
            VN = [[(k, v * nz[k]) for k, v in r] for r in V]
            Cv = [[sum(FC[i][k] * v for k, v in F[j]) + sum(vn * Vd[j][k] for k, vn in VN[i] if k in Vd[j]) for j in range(15)] for i in range(15)]
            if state is not None:
                Rn = _mm(wR, quat_R([w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, one]))
                wa0, wa1 = _mv(wR, a0b), _mv(Rn, a1b)
                am = [half * ((x - g) + (y - g)) for x, y, g in zip(wa0, wa1, grav)]
                wP = [p + dt * v + half * dt * dt * a for p, v, a in zip(wP, wV, am)]
                wV = [v + dt * a for v, a in zip(wV, am)]
                wR = Rn
            nrm = (rq[0] * rq[0] + rq[1] * rq[1] + rq[2] * rq[2] + rq[3] * rq[3]).sqrt()
            dq = [x / nrm for x in rq]; dp, dv = rp, rv
            sum_dt += dt; a0, g0 = a1, g1
            if n + 1 in snapshots:
                at[n + 1] = result(n + 1)
        out = result(len(dts))
        out["at"] = at
        return out


def preintegrate_mpmath(interval, noise=NOISE):
    """The same recursion with dense 15 x 15 and 15 x 18 mpmath matrices at 60 digits, written from the rule and sharing no step code with
    preintegrate_hp: the check of the Decimal engine (short intervals only: it is slow)."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(DPS):
        M = lambda a: mp.matrix([[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(a)])
        vec = lambda a: mp.matrix([mp.mpf(float(x)) for x in a])
        R_of = lambda q: mp.matrix(quat_R(list(q)))
        sk = lambda v: mp.matrix(_skew(list(v)))
        ba, bg, a0, g0 = vec(interval["ba"]), vec(interval["bg"]), vec(interval["acc_0"]), vec(interval["gyr_0"])
        sig = [noise[0], noise[1], noise[0], noise[1], noise[2], noise[3]]
        N = mp.diag([mp.mpf(float(sig[k // 3])) ** 2 for k in range(18)])
        dp, dv, dq, sum_dt = mp.zeros(3, 1), mp.zeros(3, 1), [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)], mp.mpf(0)
        J, Cv, I3 = mp.eye(15), mp.zeros(15), mp.eye(3)
        for dt_, a1_, g1_ in zip(np.atleast_1d(interval["dt"]), np.asarray(interval["acc"]).reshape(-1, 3), np.asarray(interval["gyr"]).reshape(-1, 3)):
            dt, a1, g1 = mp.mpf(float(dt_)), vec(a1_), vec(g1_)
            w = (g0 + g1) / 2 - bg
            Rq = R_of(dq)
            rq = quat_mul(dq, [w[0] * dt / 2, w[1] * dt / 2, w[2] * dt / 2, mp.mpf(1)])
            Rr = R_of(rq)
            un = (Rq * (a0 - ba) + Rr * (a1 - ba)) / 2
            rp = dp + dv * dt + un * dt * dt / 2; rv = dv + un * dt
            Rw, Ra0, Ra1 = sk(w), sk(a0 - ba), sk(a1 - ba)
            F, V = mp.zeros(15), mp.zeros(15, 18)
            T = I3 - Rw * dt
            F[0:3, 0:3] = I3; F[0:3, 3:6] = -(Rq * Ra0 + Rr * Ra1 * T) * dt * dt / 4; F[0:3, 6:9] = I3 * dt
            F[0:3, 9:12] = -(Rq + Rr) * dt * dt / 4; F[0:3, 12:15] = Rr * Ra1 * dt * dt * dt / 4
            F[3:6, 3:6] = T; F[3:6, 12:15] = -I3 * dt
            F[6:9, 3:6] = -(Rq * Ra0 + Rr * Ra1 * T) * dt / 2; F[6:9, 6:9] = I3; F[6:9, 9:12] = -(Rq + Rr) * dt / 2; F[6:9, 12:15] = Rr * Ra1 * dt * dt / 2
            F[9:12, 9:12] = I3; F[12:15, 12:15] = I3
            V[0:3, 0:3] = Rq * dt * dt / 4; V[0:3, 3:6] = -Rr * Ra1 * dt * dt * dt / 8; V[0:3, 6:9] = Rr * dt * dt / 4; V[0:3, 9:12] = V[0:3, 3:6]
            V[3:6, 3:6] = I3 * dt / 2; V[3:6, 9:12] = I3 * dt / 2
            V[6:9, 0:3] = Rq * dt / 2; V[6:9, 3:6] = -Rr * Ra1 * dt * dt / 4; V[6:9, 6:9] = Rr * dt / 2; V[6:9, 9:12] = V[6:9, 3:6]
            V[9:12, 12:15] = I3 * dt; V[12:15, 15:18] = I3 * dt
            J = F * J; Cv = F * Cv * F.T + V * N * V.T
            nrm = mp.sqrt(sum(x * x for x in rq))
            dq = [x / nrm for x in rq]; dp, dv = rp, rv
            sum_dt += dt; a0, g0 = a1, g1
        S = lambda x: mpmath.nstr(x, DPS + 5)
        return dict(dp=[S(x) for x in dp], dq=[S(x) for x in dq], dv=[S(x) for x in dv], J=[[S(J[i, j]) for j in range(15)] for i in range(15)],
                    C=[[S(Cv[i, j]) for j in range(15)] for i in range(15)], sum_dt=S(sum_dt))


# ------------------------------------------------------------------------------------------------ the numpy statements
def preintegrate_synth(interval):
    """synth.PreIntegration over the interval -> its block dict (the restatement whose error is E_ref)."""
    pre = synth.PreIntegration(interval["acc_0"], interval["gyr_0"], interval["ba"], interval["bg"])
    for dt, a, g in zip(np.atleast_1d(interval["dt"]), np.asarray(interval["acc"]).reshape(-1, 3), np.asarray(interval["gyr"]).reshape(-1, 3)):
        pre.push_back(float(dt), a, g)
    return pre.as_block(interval.get("frame_i", 0))


def preintegrate_np(interval, noise=NOISE, defect=None):
    """A copy of synth.PreIntegration.push_back with one switch per planted defect (DEFECTS); defect=None is the restatement itself."""
    skew, I3 = synth.skew, np.eye(3)
    ba, bg = np.array(interval["ba"], float), np.array(interval["bg"], float)
    a0, g0 = np.array(interval["acc_0"], float), np.array(interval["gyr_0"], float)
    sig = [noise[0], noise[1], noise[0], noise[1], noise[2], noise[3]]
    if defect == "noise_slots":
        sig = [noise[0], noise[1], noise[2], noise[3], noise[0], noise[1]]
    N = np.zeros((18, 18))
    for k in range(6):
        N[3 * k:3 * k + 3, 3 * k:3 * k + 3] = sig[k] ** 2 * np.eye(3)
    J, Cv, sum_dt = np.eye(15), np.zeros((15, 15)), 0.0
    dp, dv, dq = np.zeros(3), np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])
    for dt, a1, g1 in zip(np.atleast_1d(interval["dt"]), np.asarray(interval["acc"], float).reshape(-1, 3), np.asarray(interval["gyr"], float).reshape(-1, 3)):
        dt = float(dt)
        Rq = synth.quat_to_R(dq)
        un_acc_0 = Rq @ (a0 - ba)
        un_gyr = 0.5 * (g0 + g1) - (0.0 if defect == "gyr_bias" else bg)
        rq = synth.quat_mul(dq, np.array([un_gyr[0] * dt / 2, un_gyr[1] * dt / 2, un_gyr[2] * dt / 2, 1.0]))
        Rr = synth.quat_to_R_raw(rq)
        un_acc = 0.5 * (un_acc_0 + Rr @ (a1 - ba))
        rp = dp + dv * dt + 0.5 * un_acc * dt * dt
        rv = dv + un_acc * dt
        Rw, Ra0, Ra1 = skew(un_gyr), skew(a0 - ba), skew(a1 - ba)
        F = np.zeros((15, 15))
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = -0.25 * Rq @ Ra0 * dt * dt + -0.25 * Rr @ Ra1 @ (I3 - Rw * dt) * dt * dt
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -0.25 * (Rq + Rr) * dt * dt
        F[0:3, 12:15] = -0.25 * Rr @ Ra1 * dt * dt * -dt
        if defect == "F012_sign":
            F[0:3, 12:15] = -F[0:3, 12:15]
        F[3:6, 3:6] = I3 - Rw * dt
        F[3:6, 12:15] = -1.0 * I3 * dt
        F[6:9, 3:6] = -0.5 * Rq @ Ra0 * dt + -0.5 * Rr @ Ra1 @ (I3 - Rw * dt) * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -0.5 * (Rq + Rr) * dt
        F[6:9, 12:15] = -0.5 * Rr @ Ra1 * dt * -dt
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18))
        V[0:3, 0:3] = 0.25 * Rq * dt * dt
        V[0:3, 3:6] = 0.25 * -Rr @ Ra1 * dt * dt * (1.0 if defect == "v03_half_dt" else 0.5 * dt)
        V[0:3, 6:9] = 0.25 * Rr * dt * dt
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = 0.5 * I3 * dt
        V[3:6, 9:12] = 0.5 * I3 * dt
        V[6:9, 0:3] = 0.5 * Rq * dt
        V[6:9, 3:6] = 0.5 * -Rr @ Ra1 * dt * 0.5 * dt
        V[6:9, 6:9] = 0.5 * (Rq if defect == "V66_Rq" else Rr) * dt
        V[6:9, 9:12] = V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        J = F @ J
        Cv = F @ Cv @ F.T + V @ N @ V.T
        dp, dv = rp, rv
        dq = rq if defect == "no_normalise" else rq / np.linalg.norm(rq)
        sum_dt += dt
        a0, g0 = a1, g1
    return dict(sum_dt=sum_dt, delta_p=dp, delta_q=dq, delta_v=dv, linearized_ba=ba, linearized_bg=bg, jacobian=J, covariance=Cv,
                frame_i=interval.get("frame_i", 0), skip=int(sum_dt > 10.0))


def dead_reckon_np(interval, state, gravity):
    """numpy restatement of the host mirror's Estimator::deadReckon over the interval -> (P, R, V) of frame j."""
    P, R, V = np.array(state[0], float), np.array(state[1], float).reshape(3, 3), np.array(state[2], float)
    G = np.asarray(gravity, float)
    ba, bg = np.array(interval["ba"], float), np.array(interval["bg"], float)
    a0, g0 = np.array(interval["acc_0"], float), np.array(interval["gyr_0"], float)
    for dt, a1, g1 in zip(np.atleast_1d(interval["dt"]), np.asarray(interval["acc"], float).reshape(-1, 3), np.asarray(interval["gyr"], float).reshape(-1, 3)):
        dt = float(dt)
        rate = 0.5 * (g0 + g1) - bg
        th = rate * dt
        Rn = R @ synth.quat_to_R_raw(np.array([th[0] / 2.0, th[1] / 2.0, th[2] / 2.0, 1.0]))
        a_mean = 0.5 * ((R @ (a0 - ba) - G) + (Rn @ (a1 - ba) - G))
        P = P + dt * V + 0.5 * dt * dt * a_mean
        V = V + dt * a_mean
        R = Rn
        a0, g0 = a1, g1
    return P, R, V


# ------------------------------------------------------------------------------------------------ metrics
def _diff(got, hp):
    """|got - hp| as floats, the subtraction in 60 digits."""
    got = np.asarray(got, float); flat = np.asarray(hp, object).reshape(-1)
    with decimal.localcontext() as ctx:
        ctx.prec = DPS
        return np.array([float(abs(D(float(g)) - h)) for g, h in zip(got.reshape(-1), flat)]).reshape(got.shape)


def _f(hp):
    return np.array([float(x) for x in np.asarray(hp, object).reshape(-1)]).reshape(np.asarray(hp, object).shape)


def errors(block, hp):
    """The metrics of one block (a dict or a structured record with the fields of uvs_imu_block) against its 60-digit values -> dict:
    dp, dv (max-norm error over the max-norm of the vector), dq (max component error after sign alignment), J (per 3 x 3 block, max entry error over
    the block's largest entry; the largest over the blocks), C (|C - C_hp|_ij / sqrt(C_hp,ii C_hp,jj)), asym (|C - C^T| likewise),
    sum_dt (error in units of 2^-53 * sum_dt, to be held to the sample count), structure (entries of J that are exactly 0 or 1 at 60 digits and
    differ on the block: a count)."""
    out = {}
    for key, name in (("dp", "delta_p"), ("dv", "delta_v")):
        ref = np.abs(_f(hp[key])).max()
        d = _diff(block[name], hp[key]).max()
        out[key] = d / ref if ref > 0 else d
    q = np.asarray(block["delta_q"], float); qh = _f(hp["dq"])
    out["dq"] = _diff(q if np.dot(q, qh) >= 0 else -q, hp["dq"]).max()
    Jg = np.asarray(block["jacobian"], float).reshape(15, 15); Jh = _f(hp["J"]); dJ = _diff(Jg, hp["J"])
    eJ = 0.0
    for rb in range(5):
        for cb in range(5):
            s = np.s_[3 * rb:3 * rb + 3, 3 * cb:3 * cb + 3]
            top = np.abs(Jh[s]).max()
            if top > 0:
                eJ = max(eJ, dJ[s].max() / top)
    out["J"] = eJ
    exact = np.array([[h == 0 or h == 1 for h in row] for row in hp["J"]])
    out["structure"] = int(np.sum(exact & (Jg != Jh)))
    Cg = np.asarray(block["covariance"], float).reshape(15, 15); Ch = _f(hp["C"])
    dC = _diff(Cg, hp["C"]); d = np.sqrt(np.diag(Ch))
    if np.all(d > 0):
        scale = np.outer(d, d)
        out["C"] = (dC / scale).max(); out["asym"] = (np.abs(Cg - Cg.T) / scale).max()
    else:                                                     # the empty pre-integration: zero is zero
        out["C"] = dC.max(); out["asym"] = np.abs(Cg - Cg.T).max()
    sh = float(hp["sum_dt"])
    out["sum_dt"] = _diff(block["sum_dt"], [hp["sum_dt"]]).max() / (EPS * sh) if sh > 0 else abs(float(block["sum_dt"]))
    return out


METRICS = ("dp", "dq", "dv", "J", "C", "asym")          # held to 8 * max(E_ref, 2^-53); sum_dt and structure have rules of their own
DR_METRICS = ("pP", "pR", "pV")


def dr_errors(P, R, V, hp):
    """pred_p, pred_v: max-norm error over the max-norm of the 60-digit vector; pred_R: max entry error."""
    return dict(pP=_diff(P, hp["pP"]).max() / np.abs(_f(hp["pP"])).max(), pR=_diff(np.asarray(R, float).reshape(3, 3), hp["pR"]).max(),
                pV=_diff(V, hp["pV"]).max() / np.abs(_f(hp["pV"])).max())


def within(err, e_ref, n):
    """The names of the metrics of `err` (errors / dr_errors) that miss the bound 8 * max(E_ref, 2^-53), the sum_dt rule (one rounding per
    sample) or the structure rule."""
    bad = [m for m in err if m in e_ref and not err[m] <= 8.0 * max(e_ref[m], EPS)]
    if "sum_dt" in err and not err["sum_dt"] <= max(n, 0):
        bad.append("sum_dt")
    if err.get("structure", 0) != 0:
        bad.append("structure")
    return bad
