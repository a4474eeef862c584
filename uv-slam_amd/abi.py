"""ctypes mirror of include/uvs_solver.h (the C ABI of the sliding-window back-end).

Pure data-layout definitions plus helpers that turn a python-side `Window`
(numpy arrays, see synth.py) into a `uvs_window` and back.  Nothing here
computes: the arithmetic lives in csrc/ (HIP) and is reached through
libuvs_solver.so.  The same structures are used by the tests to call the CPU
oracle (oracle/liboracle.so), which shares the header.
"""
import ctypes as C
import numpy as np

WINDOW_SIZE = 10
NUM_FRAMES = WINDOW_SIZE + 1
MAX_ITER = 64
MAX_PRIOR_BLOCKS = 16
MAX_PRIOR_DIM = 96

UVS_OK, UVS_ERR_INVALID_ARG, UVS_ERR_UNSUPPORTED, UVS_ERR_NO_DEVICE, UVS_ERR_HIP, UVS_ERR_CAPACITY, UVS_ERR_NUMERIC = range(7)
UVS_BLOCK_POSE, UVS_BLOCK_SPEEDBIAS, UVS_BLOCK_EX_POSE, UVS_BLOCK_TD = range(4)      # uvs_prior.block_kind
TERM_NAMES = ["NO_CONVERGENCE", "GRADIENT_TOL", "PARAMETER_TOL", "FUNCTION_TOL", "MIN_RADIUS", "INVALID_STEPS", "NUMERIC_FAILURE"]
BLOCK_POSE, BLOCK_SPEEDBIAS, BLOCK_EX_POSE, BLOCK_TD = range(4)

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int32)


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("estimate_extrinsic", C.c_int32), ("estimate_td", C.c_int32),
        ("function_tol_keeps_candidate", C.c_int32),
        ("focal_length", C.c_double), ("point_sqrt_info", C.c_double), ("line_factor", C.c_double), ("vp_factor", C.c_double),
        ("loss_point", C.c_double), ("loss_line", C.c_double), ("loss_vp", C.c_double), ("gravity", C.c_double * 3),
        ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
        ("max_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("max_solver_time_in_seconds", C.c_double),
    ]


def default_options():
    """EuRoC values (config/euroc/euroc_config.yaml) + Ceres defaults; mirrors uvs_default_options()."""
    o = Options()
    o.max_num_iterations = 10
    o.estimate_extrinsic = 0
    o.estimate_td = 0
    o.function_tol_keeps_candidate = 0
    o.focal_length = 461.6
    o.point_sqrt_info = 461.6 / 1.6
    o.line_factor = 300.0
    o.vp_factor = 10.0
    o.loss_point, o.loss_line, o.loss_vp = 1.0, 0.1, 1.0
    o.gravity[0], o.gravity[1], o.gravity[2] = 0.0, 0.0, 9.81007
    o.initial_trust_region_radius = 1e4
    o.max_trust_region_radius = 1e16
    o.min_trust_region_radius = 1e-32
    o.min_relative_decrease = 1e-3
    o.min_lm_diagonal = 1e-6
    o.max_lm_diagonal = 1e32
    o.function_tolerance = 1e-6
    o.gradient_tolerance = 1e-10
    o.parameter_tolerance = 1e-8
    o.max_consecutive_invalid_steps = 5
    o.jacobi_scaling = 1
    return o


class ImuBlock(C.Structure):
    _fields_ = [
        ("sum_dt", C.c_double), ("delta_p", C.c_double * 3), ("delta_q", C.c_double * 4), ("delta_v", C.c_double * 3),
        ("linearized_ba", C.c_double * 3), ("linearized_bg", C.c_double * 3),
        ("jacobian", C.c_double * 225), ("covariance", C.c_double * 225),
        ("frame_i", C.c_int32), ("skip", C.c_int32),
    ]


class Prior(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("n_blocks", C.c_int32),
        ("block_kind", C.c_int32 * MAX_PRIOR_BLOCKS), ("block_frame", C.c_int32 * MAX_PRIOR_BLOCKS),
        ("block_size", C.c_int32 * MAX_PRIOR_BLOCKS), ("block_idx", C.c_int32 * MAX_PRIOR_BLOCKS),
        ("x0_off", C.c_int32 * MAX_PRIOR_BLOCKS),
        ("x0", C.c_double * (MAX_PRIOR_BLOCKS * 9)),
        ("linearized_residuals", C.c_double * MAX_PRIOR_DIM),
        ("linearized_jacobians", C.c_double * (MAX_PRIOR_DIM * MAX_PRIOR_DIM)),
    ]

    def J0(self):
        n = self.n
        return np.ctypeslib.as_array(self.linearized_jacobians)[: n * n].reshape(n, n).copy()

    def r0(self):
        return np.ctypeslib.as_array(self.linearized_residuals)[: self.n].copy()

    def copy(self):
        p = Prior()
        C.memmove(C.byref(p), C.byref(self), C.sizeof(Prior))
        return p


class WindowC(C.Structure):
    _fields_ = [
        ("pose", (C.c_double * 7) * NUM_FRAMES), ("speedbias", (C.c_double * 9) * NUM_FRAMES), ("ex_pose", C.c_double * 7),
        ("td", C.c_double),
        ("n_points", C.c_int32), ("n_point_obs", C.c_int32),
        ("inv_depth", c_double_p), ("pt_lm", c_int_p), ("pt_fi", c_int_p), ("pt_fj", c_int_p), ("pt_pi", c_double_p), ("pt_pj", c_double_p),
        ("n_lines", C.c_int32), ("n_line_obs", C.c_int32),
        ("line_orth", c_double_p), ("ln_lm", c_int_p), ("ln_fj", c_int_p), ("ln_sp", c_double_p), ("ln_ep", c_double_p),
        ("ln_has_vp", c_int_p), ("ln_vp", c_double_p),
        ("n_imu", C.c_int32), ("imu", C.POINTER(ImuBlock)),
        ("prior", C.POINTER(Prior)),
        ("pt_vel_i", c_double_p), ("pt_vel_j", c_double_p), ("pt_td_i", c_double_p), ("pt_td_j", c_double_p),
        ("n_relo_obs", C.c_int32), ("relo_pose", C.c_double * 7), ("relo_lm", c_int_p), ("relo_pi", c_double_p), ("relo_pj", c_double_p),
    ]


class StateC(C.Structure):
    _fields_ = [
        ("pose", (C.c_double * 7) * NUM_FRAMES), ("speedbias", (C.c_double * 9) * NUM_FRAMES), ("ex_pose", C.c_double * 7),
        ("td", C.c_double), ("inv_depth", c_double_p), ("line_orth", c_double_p), ("relo_pose", C.c_double * 7),
    ]


class Report(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("termination", C.c_int32), ("num_iterations", C.c_int32), ("num_successful", C.c_int32),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("cost", C.c_double * (MAX_ITER + 1)), ("candidate_cost", C.c_double * (MAX_ITER + 1)),
        ("model_cost_change", C.c_double * (MAX_ITER + 1)), ("relative_decrease", C.c_double * (MAX_ITER + 1)),
        ("radius", C.c_double * (MAX_ITER + 1)), ("step_norm", C.c_double * (MAX_ITER + 1)),
        ("gradient_max_norm", C.c_double * (MAX_ITER + 1)), ("accepted", C.c_int32 * (MAX_ITER + 1)),
    ]

    def trace(self):
        k = self.num_iterations + 1
        f = lambda a: np.array(a[:k])
        return dict(cost=f(self.cost), candidate_cost=f(self.candidate_cost), model_cost_change=f(self.model_cost_change),
                    relative_decrease=f(self.relative_decrease), radius=f(self.radius), step_norm=f(self.step_norm),
                    gradient_max_norm=f(self.gradient_max_norm), accepted=np.array(self.accepted[:k]))


class EvalC(C.Structure):
    _fields_ = [
        ("pt_r", c_double_p), ("pt_J", c_double_p), ("ln_r", c_double_p), ("ln_J", c_double_p), ("vp_r", c_double_p), ("vp_J", c_double_p),
        ("imu_r", c_double_p), ("imu_J", c_double_p), ("prior_r", c_double_p), ("cost", C.c_double), ("pt_Jtd", c_double_p),
    ]


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


class Window:
    """Python-side sliding window: numpy mirrors of the para_* arrays and the factor lists.

    Field meanings and reference citations are those of `uvs_window` in include/uvs_solver.h.
    """

    def __init__(self):
        self.pose = np.zeros((NUM_FRAMES, 7)); self.pose[:, 6] = 1.0
        self.speedbias = np.zeros((NUM_FRAMES, 9))
        self.ex_pose = np.zeros(7); self.ex_pose[6] = 1.0
        self.td = 0.0
        self.inv_depth = np.zeros(0)
        self.pt_lm = np.zeros(0, np.int32); self.pt_fi = np.zeros(0, np.int32); self.pt_fj = np.zeros(0, np.int32)
        self.pt_pi = np.zeros((0, 3)); self.pt_pj = np.zeros((0, 3))
        self.pt_vel_i = None; self.pt_vel_j = None; self.pt_td_i = None; self.pt_td_j = None      # ProjectionTdFactor inputs (estimate_td), [n_obs,2] / [n_obs]
        # relocalization blocks (estimator.cpp:944-978): landmark index, pts_i (first observation), pts_j (match point); relo_Pose
        self.relo_pose = np.zeros(7); self.relo_pose[6] = 1.0
        self.relo_frame = 0    # relo_frame_local_index: not an input of the solve (Estimator::double2vector reads it), carried by the window file
        self.relo_lm = np.zeros(0, np.int32); self.relo_pi = np.zeros((0, 3)); self.relo_pj = np.zeros((0, 3))
        self.line_orth = np.zeros((0, 4))
        self.ln_lm = np.zeros(0, np.int32); self.ln_fj = np.zeros(0, np.int32)
        self.ln_sp = np.zeros((0, 3)); self.ln_ep = np.zeros((0, 3))
        self.ln_has_vp = np.zeros(0, np.int32); self.ln_vp = np.zeros((0, 3))
        self.imu = []          # list of dict(sum_dt, delta_p, delta_q, delta_v, linearized_ba, linearized_bg, jacobian(15,15), covariance(15,15), frame_i, skip)
        self.prior = None      # abi.Prior or None
        self.truth = None      # optional dict with ground-truth state (synthetic windows)

    # -- conversion ---------------------------------------------------------
    def to_c(self):
        """Returns (WindowC, keepalive) -- keepalive must outlive every use of the struct."""
        k = {}
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        w = WindowC()
        pose, sb, ex = f64(self.pose), f64(self.speedbias), f64(self.ex_pose)
        C.memmove(w.pose, pose.ctypes.data, pose.nbytes)
        C.memmove(w.speedbias, sb.ctypes.data, sb.nbytes)
        C.memmove(w.ex_pose, ex.ctypes.data, ex.nbytes)
        w.td = float(self.td)
        for name in ("inv_depth", "pt_pi", "pt_pj", "line_orth", "ln_sp", "ln_ep", "ln_vp"):
            k[name] = f64(getattr(self, name)); setattr(w, name, _dp(k[name]))
        for name in ("pt_lm", "pt_fi", "pt_fj", "ln_lm", "ln_fj", "ln_has_vp"):
            k[name] = i32(getattr(self, name)); setattr(w, name, _ip(k[name]))
        for name in ("pt_vel_i", "pt_vel_j", "pt_td_i", "pt_td_j"):
            if getattr(self, name) is not None:
                k[name] = f64(getattr(self, name)); setattr(w, name, _dp(k[name]))
        k["relo_lm"] = i32(self.relo_lm); k["relo_pi"] = f64(self.relo_pi); k["relo_pj"] = f64(self.relo_pj); relo = f64(self.relo_pose)
        w.n_relo_obs = len(k["relo_lm"]); w.relo_lm = _ip(k["relo_lm"]); w.relo_pi = _dp(k["relo_pi"]); w.relo_pj = _dp(k["relo_pj"])
        C.memmove(w.relo_pose, relo.ctypes.data, relo.nbytes)
        w.n_points = len(k["inv_depth"]); w.n_point_obs = len(k["pt_lm"])
        w.n_lines = len(k["line_orth"]); w.n_line_obs = len(k["ln_lm"])
        n_imu = len(self.imu)
        arr = (ImuBlock * max(n_imu, 1))()
        for b, d in enumerate(self.imu):
            ib = arr[b]
            ib.sum_dt = float(d["sum_dt"])
            for name, n in (("delta_p", 3), ("delta_q", 4), ("delta_v", 3), ("linearized_ba", 3), ("linearized_bg", 3)):
                v = f64(d[name]).ravel(); assert v.size == n
                C.memmove(getattr(ib, name), v.ctypes.data, v.nbytes)
            for name in ("jacobian", "covariance"):
                v = f64(d[name]).reshape(225)
                C.memmove(getattr(ib, name), v.ctypes.data, v.nbytes)
            ib.frame_i = int(d["frame_i"]); ib.skip = int(d.get("skip", 0))
        k["imu"] = arr
        w.n_imu = n_imu
        w.imu = C.cast(arr, C.POINTER(ImuBlock))
        if self.prior is not None and self.prior.n > 0:
            k["prior"] = self.prior
            w.prior = C.pointer(self.prior)
        else:
            w.prior = None
        return w, k

    # -- record / replay file (layout documented in host/window_io.h) ------------
    def save(self, path):
        f64 = lambda a: np.ascontiguousarray(a, dtype="<f8").tobytes()
        i32 = lambda a: np.ascontiguousarray(a, dtype="<i4").tobytes()
        npo, nlo = len(self.pt_lm), len(self.ln_lm)
        pn = self.prior.n if self.prior is not None else 0
        pnb = self.prior.n_blocks if pn else 0
        with open(path, "wb") as f:
            f.write(b"UVSWIN01")
            has_td = self.pt_vel_i is not None
            nrl = len(self.relo_lm)
            f.write(i32([len(self.inv_depth), npo, len(self.line_orth), nlo, len(self.imu), pn, pnb, (1 if has_td else 0) | (2 if nrl else 0)]))
            f.write(f64(self.pose)); f.write(f64(self.speedbias)); f.write(f64(self.ex_pose)); f.write(f64([self.td]))
            f.write(f64(self.inv_depth))
            f.write(i32(self.pt_lm)); f.write(i32(self.pt_fi)); f.write(i32(self.pt_fj))
            if npo % 2: f.write(i32([0]))
            f.write(f64(self.pt_pi)); f.write(f64(self.pt_pj))
            if has_td:      # ProjectionTdFactor inputs (header word 8 = 1)
                f.write(f64(self.pt_vel_i)); f.write(f64(self.pt_vel_j)); f.write(f64(self.pt_td_i)); f.write(f64(self.pt_td_j))
            f.write(f64(self.line_orth))
            f.write(i32(self.ln_lm)); f.write(i32(self.ln_fj)); f.write(i32(self.ln_has_vp))
            if nlo % 2: f.write(i32([0]))
            f.write(f64(self.ln_sp)); f.write(f64(self.ln_ep)); f.write(f64(self.ln_vp))
            for b in self.imu:
                f.write(f64([b["sum_dt"]])); f.write(f64(b["delta_p"])); f.write(f64(b["delta_q"])); f.write(f64(b["delta_v"]))
                f.write(f64(b["linearized_ba"])); f.write(f64(b["linearized_bg"])); f.write(f64(np.asarray(b["jacobian"]).reshape(225)))
                f.write(f64(np.asarray(b["covariance"]).reshape(225))); f.write(i32([b["frame_i"], b.get("skip", 0)]))
            if pn:
                p = self.prior
                for name in ("block_kind", "block_frame", "block_size", "block_idx", "x0_off"):
                    f.write(i32(list(getattr(p, name))))
                f.write(f64(list(p.x0))); f.write(f64(p.r0())); f.write(f64(p.J0()))
            if nrl:         # relocalization section (header word 8, bit 1): count, relo_frame_local_index, relo_Pose, landmark indices (+pad), pts_i, pts_j
                f.write(i32([nrl, int(self.relo_frame)])); f.write(f64(self.relo_pose)); f.write(i32(self.relo_lm))
                if nrl % 2: f.write(i32([0]))
                f.write(f64(self.relo_pi)); f.write(f64(self.relo_pj))

    @staticmethod
    def load(path):
        """Reads a window file (the layout of save() / host/window_io.h), e.g. one written by the UVS_DUMP_WINDOWS record hook."""
        buf = open(path, "rb").read()
        if buf[:8] != b"UVSWIN01": raise ValueError("not a window file: %s" % path)
        pos = [8]

        def take(dtype, n):
            a = np.frombuffer(buf, dtype=dtype, count=n, offset=pos[0]).copy(); pos[0] += a.nbytes; return a

        np_, npo, nl, nlo, ni, pn, pnb, flags = (int(v) for v in take("<i4", 8))
        has_td, has_relo = flags & 1, flags & 2
        # header counts are untrusted: the prior lands in fixed-size ctypes arrays
        if min(np_, npo, nl, nlo, ni, pn, pnb) < 0 or ni > NUM_FRAMES - 1 or pn > MAX_PRIOR_DIM or pnb > MAX_PRIOR_BLOCKS:
            raise ValueError("corrupt window file header: %s" % path)
        w = Window()
        w.pose = take("<f8", 77).reshape(NUM_FRAMES, 7); w.speedbias = take("<f8", 99).reshape(NUM_FRAMES, 9); w.ex_pose = take("<f8", 7); w.td = float(take("<f8", 1)[0])
        w.inv_depth = take("<f8", np_)
        w.pt_lm, w.pt_fi, w.pt_fj = take("<i4", npo), take("<i4", npo), take("<i4", npo)
        if npo % 2: take("<i4", 1)
        w.pt_pi = take("<f8", 3 * npo).reshape(-1, 3); w.pt_pj = take("<f8", 3 * npo).reshape(-1, 3)
        if has_td:
            w.pt_vel_i = take("<f8", 2 * npo).reshape(-1, 2); w.pt_vel_j = take("<f8", 2 * npo).reshape(-1, 2); w.pt_td_i = take("<f8", npo); w.pt_td_j = take("<f8", npo)
        w.line_orth = take("<f8", 4 * nl).reshape(-1, 4)
        w.ln_lm, w.ln_fj, w.ln_has_vp = take("<i4", nlo), take("<i4", nlo), take("<i4", nlo)
        if nlo % 2: take("<i4", 1)
        w.ln_sp = take("<f8", 3 * nlo).reshape(-1, 3); w.ln_ep = take("<f8", 3 * nlo).reshape(-1, 3); w.ln_vp = take("<f8", 3 * nlo).reshape(-1, 3)
        for _ in range(ni):
            h = take("<f8", 17); jac = take("<f8", 225).reshape(15, 15); cov = take("<f8", 225).reshape(15, 15); fs = take("<i4", 2)
            w.imu.append(dict(sum_dt=float(h[0]), delta_p=h[1:4], delta_q=h[4:8], delta_v=h[8:11], linearized_ba=h[11:14], linearized_bg=h[14:17],
                              jacobian=jac, covariance=cov, frame_i=int(fs[0]), skip=int(fs[1])))
        if pn > 0:
            p = Prior(); p.n = pn; p.n_blocks = pnb
            for name in ("block_kind", "block_frame", "block_size", "block_idx", "x0_off"):
                v = take("<i4", 16)
                for k in range(16): getattr(p, name)[k] = int(v[k])
            x0 = take("<f8", 144); r0 = take("<f8", pn); J0 = take("<f8", pn * pn)
            for k in range(144): p.x0[k] = x0[k]
            C.memmove(p.linearized_residuals, r0.ctypes.data, r0.nbytes); C.memmove(p.linearized_jacobians, J0.ctypes.data, J0.nbytes)
            w.prior = p
        if has_relo:
            nrl, w.relo_frame = (int(v) for v in take("<i4", 2)); w.relo_pose = take("<f8", 7); w.relo_lm = take("<i4", nrl)
            if nrl % 2: take("<i4", 1)
            w.relo_pi = take("<f8", 3 * nrl).reshape(-1, 3); w.relo_pj = take("<f8", 3 * nrl).reshape(-1, 3)
        return w

    def copy(self):
        import copy
        o = Window()
        for name, v in self.__dict__.items():
            if isinstance(v, np.ndarray):
                setattr(o, name, v.copy())
            elif name == "prior":
                o.prior = v.copy() if v is not None else None
            else:
                setattr(o, name, copy.deepcopy(v))
        return o

    def with_state(self, st):
        """New window whose state is `st` (a State), factors unchanged."""
        o = self.copy()
        o.pose = st.pose.copy(); o.speedbias = st.speedbias.copy(); o.ex_pose = st.ex_pose.copy()
        o.inv_depth = st.inv_depth.copy(); o.line_orth = st.line_orth.copy()
        o.td = float(getattr(st, "td", o.td))
        return o


class State:
    """Solver output (para_* arrays after the solve, before double2vector)."""

    def __init__(self, n_points, n_lines):
        self.pose = np.zeros((NUM_FRAMES, 7)); self.speedbias = np.zeros((NUM_FRAMES, 9)); self.ex_pose = np.zeros(7)
        self.td = 0.0
        self.relo_pose = np.zeros(7)
        self.inv_depth = np.zeros(n_points); self.line_orth = np.zeros((n_lines, 4))

    def alloc_c(self):
        s = StateC()
        s.inv_depth = _dp(self.inv_depth)
        s.line_orth = _dp(self.line_orth)
        return s

    def from_c(self, s):
        self.pose = np.array(s.pose).reshape(NUM_FRAMES, 7)
        self.speedbias = np.array(s.speedbias).reshape(NUM_FRAMES, 9)
        self.ex_pose = np.array(s.ex_pose)
        self.td = s.td
        self.relo_pose = np.array(s.relo_pose)
        return self


class Eval:
    def __init__(self, w: Window):
        npo, nlo, ni = len(w.pt_lm), len(w.ln_lm), len(w.imu)
        n = w.prior.n if w.prior is not None else 0
        self.pt_r = np.zeros((npo, 2)); self.pt_J = np.zeros((npo, 2, 19)); self.pt_Jtd = np.zeros((npo, 2))
        self.ln_r = np.zeros((nlo, 2)); self.ln_J = np.zeros((nlo, 2, 10))
        self.vp_r = np.zeros((nlo, 1)); self.vp_J = np.zeros((nlo, 1, 10))
        self.imu_r = np.zeros((ni, 15)); self.imu_J = np.zeros((ni, 15, 30))
        self.prior_r = np.zeros(max(n, 1))
        self.cost = 0.0

    def alloc_c(self):
        e = EvalC()
        for name in ("pt_r", "pt_J", "ln_r", "ln_J", "vp_r", "vp_J", "imu_r", "imu_J", "prior_r", "pt_Jtd"):
            setattr(e, name, _dp(getattr(self, name)))
        return e


# ---- 4-DoF pose graph of loop closure (uvs_pg_*, include/uvs_solver.h) ------------------------------------------------
PG_MAX_KEYFRAMES = 65536
PG_MAX_LOOPS = 256
PG_DEBUG_SCAL_LEN = 4


class PgLoop(C.Structure):
    _fields_ = [("cur", C.c_int32), ("old", C.c_int32), ("rel_t", C.c_double * 3), ("rel_yaw", C.c_double)]


class PgProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_loops", C.c_int32), ("t", c_double_p), ("q", c_double_p), ("sequence", c_int_p), ("constant", c_int_p),
                ("loops", C.POINTER(PgLoop))]


class PgReport(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("termination", C.c_int32), ("num_iterations", C.c_int32), ("num_successful", C.c_int32),
        ("n_free", C.c_int32), ("n_edges", C.c_int32), ("n_loop_columns", C.c_int32), ("reserved", C.c_int32),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("cost", C.c_double * (MAX_ITER + 1)), ("candidate_cost", C.c_double * (MAX_ITER + 1)),
        ("model_cost_change", C.c_double * (MAX_ITER + 1)), ("radius", C.c_double * (MAX_ITER + 1)),
        ("accepted", C.c_int32 * (MAX_ITER + 1)),
    ]

    def trace(self):
        k = self.num_iterations + 1
        f = lambda a: np.array(a[:k])
        return dict(cost=f(self.cost), candidate_cost=f(self.candidate_cost), model_cost_change=f(self.model_cost_change), radius=f(self.radius),
                    accepted=np.array(self.accepted[:k]))


def pg_problem(t, q, sequence, constant, loops):
    """(PgProblem, keepalive).  t [n,3], q [n,4] (x,y,z,w), sequence / constant [n], loops = iterable of (cur, old, rel_t[3], rel_yaw)."""
    k = dict(t=np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3), q=np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 4),
             sequence=np.ascontiguousarray(sequence, dtype=np.int32), constant=np.ascontiguousarray(constant, dtype=np.int32))
    loops = list(loops)
    arr = (PgLoop * max(len(loops), 1))()
    for l, (cur, old, rel_t, rel_yaw) in enumerate(loops):
        arr[l].cur, arr[l].old, arr[l].rel_yaw = int(cur), int(old), float(rel_yaw)
        for c in range(3):
            arr[l].rel_t[c] = float(rel_t[c])
    k["loops"] = arr
    p = PgProblem()
    p.n, p.n_loops = len(k["t"]), len(loops)
    p.t, p.q, p.sequence, p.constant = _dp(k["t"]), _dp(k["q"]), _ip(k["sequence"]), _ip(k["constant"])
    p.loops = C.cast(arr, C.POINTER(PgLoop))
    return p, k


# ---- loop verification of loop closure (uvs_lc_*, include/uvs_solver.h) ------------------------------------------------
LC_MAX_PAIRS = 4096
LC_MAX_QUERY = 1024
LC_MAX_OLD = 4096
LC_N_HYPOTHESES = 100
LC_REASONS = ["ACCEPTED", "NO_MATCHES", "FEW_MATCHES", "RANSAC_FAILED", "FEW_INLIERS", "YAW_GATE", "T_GATE"]      # uvs_lc_result.reason
c_u64_p = C.POINTER(C.c_uint64)


class LcPair(C.Structure):
    _fields_ = [("n_query", C.c_int32), ("n_old", C.c_int32), ("p3d", c_double_p), ("desc", c_u64_p), ("vio_t", C.c_double * 3),
                ("vio_q", C.c_double * 4), ("old_uv_norm", c_double_p), ("old_desc", c_u64_p), ("seed", C.c_uint64)]


class LcResult(C.Structure):
    _fields_ = [
        ("accepted", C.c_int32), ("reason", C.c_int32), ("n_matches", C.c_int32), ("n_inliers", C.c_int32),
        ("best_hypothesis", C.c_int32), ("ransac_iters", C.c_int32),
        ("loop_info", C.c_double * 8), ("PnP_T_old", C.c_double * 3), ("PnP_q_old", C.c_double * 4),
        ("hyp_inliers", C.c_int32 * LC_N_HYPOTHESES),
    ]

    def as_dict(self):
        return dict(accepted=int(self.accepted), reason=int(self.reason), n_matches=int(self.n_matches), n_inliers=int(self.n_inliers),
                    best_hypothesis=int(self.best_hypothesis), ransac_iters=int(self.ransac_iters), loop_info=np.array(self.loop_info[:]),
                    PnP_T_old=np.array(self.PnP_T_old[:]), PnP_q_old=np.array(self.PnP_q_old[:]),
                    hyp_inliers=np.array(self.hyp_inliers[:], np.int32))


def lc_pairs(pairs):
    """(LcPair array, keepalive) from dicts with p3d [nq,3], qdesc [nq,4] uint64, vio_t [3], vio_q [4] (x,y,z,w), uv [no,2], odesc [no,4] uint64,
    seed."""
    arr = (LcPair * max(len(pairs), 1))()
    keep = []
    for b, d in enumerate(pairs):
        p3d = np.ascontiguousarray(d["p3d"], dtype=np.float64).reshape(-1, 3); qd = np.ascontiguousarray(d["qdesc"], dtype=np.uint64).reshape(-1, 4)
        uv = np.ascontiguousarray(d["uv"], dtype=np.float64).reshape(-1, 2); od = np.ascontiguousarray(d["odesc"], dtype=np.uint64).reshape(-1, 4)
        keep += [p3d, qd, uv, od]
        e = arr[b]
        e.n_query, e.n_old = len(p3d), len(uv)
        e.p3d, e.desc = _dp(p3d), qd.ctypes.data_as(c_u64_p)
        e.old_uv_norm, e.old_desc = _dp(uv), od.ctypes.data_as(c_u64_p)
        for c in range(3):
            e.vio_t[c] = float(d["vio_t"][c])
        for c in range(4):
            e.vio_q[c] = float(d["vio_q"][c])
        e.seed = int(d["seed"]) & ((1 << 64) - 1)
    return arr, keep


# the trace of uvs_lc_debug_pair (UVS_LC_TRACE_* of the header)
LC_LM_ITERS = 20
LC_TRACE_HEAD_LEN = 32
LC_TRACE_ITER_LEN = 64
LC_TRACE_REC_LEN = LC_TRACE_HEAD_LEN + LC_LM_ITERS * LC_TRACE_ITER_LEN
LC_TRACE_STAGE_OFF = (LC_N_HYPOTHESES + 1) * LC_TRACE_REC_LEN
LC_TRACE_LEN = LC_TRACE_STAGE_OFF + 1 + 6 * LC_MAX_QUERY


def lc_trace(raw):
    """The raw doubles of uvs_lc_debug_pair -> dict of views: raw; n; X [n,3], uv [n,2], mq [n] (the staged matches); per record r (0 .. 99 the
    hypotheses, 100 the refinement): samples [101,5], valid [101], iters [101], cost0 [101], pose [101,12] (final R row-major, t), drew [101],
    start [12] (the refinement's start pose), and it [101,20,64] (the iteration records: start 0:12, lambda 12, acc 13:41, chol_ok 41,
    d 42:48, cand 48:60, cc 60, cost 61, accepted 62, stop 63)."""
    raw = np.asarray(raw, np.float64)
    assert raw.shape == (LC_TRACE_LEN,)
    rec = raw[:LC_TRACE_STAGE_OFF].reshape(LC_N_HYPOTHESES + 1, LC_TRACE_REC_LEN)
    st = raw[LC_TRACE_STAGE_OFF:]
    n = int(st[0])
    Q = LC_MAX_QUERY
    return dict(raw=raw, n=n, X=st[1:1 + 3 * Q].reshape(Q, 3)[:n], uv=st[1 + 3 * Q:1 + 5 * Q].reshape(Q, 2)[:n], mq=st[1 + 5 * Q:1 + 6 * Q][:n].astype(np.int64),
                samples=rec[:, 0:5].astype(np.int64), valid=rec[:, 5].astype(np.int64), iters=rec[:, 6].astype(np.int64), cost0=rec[:, 7],
                pose=rec[:, 8:20], drew=rec[:, 20].astype(np.int64), start=rec[LC_N_HYPOTHESES, 20:32],
                it=rec[:, LC_TRACE_HEAD_LEN:].reshape(LC_N_HYPOTHESES + 1, LC_LM_ITERS, LC_TRACE_ITER_LEN))


# ---- vanishing points of the line front end (uvs_vp_*, include/uvs_solver.h) ------------------------------------------------
VP_MAX_FRAMES = 1024
VP_MAX_LINES = 1024
VP_MAX_COORD = 1e7
VP_N_SAMPLES = 105
VP_N_ROTATIONS = 360
VP_N_HYPOTHESES = VP_N_SAMPLES * VP_N_ROTATIONS
VP_GRID_LA, VP_GRID_LO = 90, 360
VP_STATUS = ["OK", "TOO_FEW_LINES", "NO_HYPOTHESIS"]      # uvs_vp_result.status


class VpFrame(C.Structure):
    _fields_ = [("n_lines", C.c_int32), ("reserved", C.c_int32), ("segments", c_double_p), ("seed", C.c_uint64)]


class VpCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class VpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("best_hypothesis", C.c_int32), ("score", C.c_double), ("vps", (C.c_double * 3) * 3),
                ("n_tagged", C.c_int32 * 3), ("reserved", C.c_int32)]

    def as_dict(self):
        return dict(status=int(self.status), best_hypothesis=int(self.best_hypothesis), score=float(self.score),
                    vps=np.array([list(r) for r in self.vps]), n_tagged=np.array(self.n_tagged[:], np.int32))


def vp_frames(frames):
    """(VpFrame array, keepalive) from dicts with segs [n, 4] (x1, y1, x2, y2 in pixels) and seed."""
    arr = (VpFrame * max(len(frames), 1))()
    keep = []
    for b, d in enumerate(frames):
        s = np.ascontiguousarray(d["segs"], dtype=np.float64).reshape(-1, 4)
        keep.append(s)
        arr[b].n_lines = len(s)
        arr[b].segments = _dp(s)
        arr[b].seed = int(d["seed"]) & ((1 << 64) - 1)
    return arr, keep


def vp_camera(cam):
    c = VpCamera()
    c.fx, c.fy, c.cx, c.cy = (float(v) for v in cam)
    return c


# ---- keyframe features of loop closure (uvs_kf_*, include/uvs_solver.h) ------------------------------------------------
KF_MAX_FRAMES = 64
KF_MIN_SIZE = 9
KF_MAX_WIDTH = 4096
KF_MAX_HEIGHT = 4096
KF_PATTERN_BITS = 256
KF_MAX_PATTERN_OFFSET = 1024
KF_MAX_COORD = 1e6
KF_STATUS = ["OK", "OVERFLOW"]      # uvs_kf_result.status
c_u8_p = C.POINTER(C.c_uint8)
c_float_p = C.POINTER(C.c_float)
c_i32_p = C.POINTER(C.c_int32)


class KfFrame(C.Structure):
    _fields_ = [("image", c_u8_p), ("width", C.c_int32), ("height", C.c_int32), ("n_window", C.c_int32), ("reserved", C.c_int32),
                ("window_uv", c_float_p)]


class KfCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class KfResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_keypoints", C.c_int32), ("n_returned", C.c_int32), ("n_corners_before_nms", C.c_int32)]

    def as_dict(self):
        return dict(status=int(self.status), n_keypoints=int(self.n_keypoints), n_returned=int(self.n_returned),
                    n_corners_before_nms=int(self.n_corners_before_nms))


def kf_frames(frames):
    """(KfFrame array, keepalive) from dicts with image [H, W] uint8 and window_uv [n, 2] float32 pixels (optional)."""
    arr = (KfFrame * max(len(frames), 1))()
    keep = []
    for b, d in enumerate(frames):
        im = np.ascontiguousarray(d["image"], dtype=np.uint8)
        uv = np.ascontiguousarray(d.get("window_uv", np.zeros((0, 2))), dtype=np.float32).reshape(-1, 2)
        keep += [im, uv]
        arr[b].image = im.ctypes.data_as(c_u8_p)
        arr[b].height, arr[b].width = im.shape
        arr[b].n_window = len(uv)
        arr[b].window_uv = uv.ctypes.data_as(c_float_p) if len(uv) else None
    return arr, keep


def kf_camera(cam):
    """(fx, fy, cx, cy) or (fx, fy, cx, cy, k1, k2, p1, p2)."""
    c = KfCamera()
    v = [float(x) for x in cam] + [0.0] * (8 - len(cam))
    c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2 = v
    return c


def load_brief_pattern(path):
    """The reference's brief_pattern.yml -> int32 [4, 256] (x1, y1, x2, y2).  The file is a flat YAML of four integer lists (`key:` then
    `  - value` lines, or an inline `[a, b, ..]`), so it is parsed here without a YAML library."""
    lists, key = {}, None
    with open(path) as f:
        for line in f:
            s = line.split("#", 1)[0].strip()
            if not s or s.startswith("%") or s == "---":
                continue
            if s.startswith("-"):
                if key is None:
                    raise ValueError(f"{path}: a list item before any key")
                lists[key] += [int(v) for v in s[1:].replace(",", " ").split()]
            elif ":" in s:
                key, rest = (t.strip() for t in s.split(":", 1))
                lists[key] = [int(v) for v in rest.strip("[]").replace(",", " ").split()]
            else:                                            # the continuation of an inline list
                lists[key] += [int(v) for v in s.strip("[]").replace(",", " ").split()]
    try:
        pat = np.array([lists[k] for k in ("x1", "y1", "x2", "y2")], dtype=np.int32)
    except (KeyError, ValueError) as e:
        raise ValueError(f"{path}: x1, y1, x2, y2 must be four integer lists of equal length") from e
    if pat.shape != (4, KF_PATTERN_BITS):
        raise ValueError(f"{path}: {pat.shape[1]} tests per list, {KF_PATTERN_BITS} expected")
    return pat


# ---- point tracking of the point front end (uvs_ft_*, include/uvs_solver.h) -----------------------------------------------
FT_MAX_STREAMS = 64
FT_MAX_LEVELS = 4
FT_MIN_SIZE = 24
FT_MAX_POINTS = 8192
FT_WINDOW = 21
FT_MAX_ITERATIONS = 30
FT_TRACE_HEADER = 16
FT_TRACE_ITER = 10
FT_TRACE_LEVEL = 320
FT_STATUS = ["TRACKED", "LOST_FLAT", "LOST_OUTSIDE", "LOST_BORDER"]      # status[] of uvs_ft_track


class FtItem(C.Structure):
    _fields_ = [("image", c_u8_p), ("stream", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_points", C.c_int32),
                ("points_xy", c_double_p)]


def ft_items(items):
    """(FtItem array, keepalive) from dicts with stream, image [H, W] uint8 and points [n, 2] float64 pixels of the slot's previous image
    (optional)."""
    arr = (FtItem * max(len(items), 1))()
    keep = []
    for b, d in enumerate(items):
        im = np.ascontiguousarray(d["image"], dtype=np.uint8)
        pts = np.ascontiguousarray(d.get("points", np.zeros((0, 2))), dtype=np.float64).reshape(-1, 2)
        keep += [im, pts]
        arr[b].image = im.ctypes.data_as(c_u8_p)
        arr[b].stream = int(d.get("stream", 0))
        arr[b].height, arr[b].width = im.shape
        arr[b].n_points = len(pts)
        arr[b].points_xy = pts.ctypes.data_as(c_double_p) if len(pts) else None
    return arr, keep


# ---- new points of the point front end (uvs_ft_detect, include/uvs_solver.h) ---------------------------------------------
FT_DEFAULT_CANDIDATES = 65536
FT_MAX_CANDIDATES = 1 << 20
FT_MAX_MIN_DISTANCE = 1024
FT_DETECT_OK, FT_DETECT_OVERFLOW = 0, 1


class FtDetectItem(C.Structure):
    _fields_ = [("stream", C.c_int32), ("n_occupied", C.c_int32), ("max_new", C.c_int32), ("reserved", C.c_int32), ("occupied_xy", c_double_p)]


class FtDetectResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_new", C.c_int32), ("n_candidates", C.c_int32), ("reserved", C.c_int32),
                ("max_score", C.c_double), ("threshold", C.c_double)]


def ft_detect_items(items):
    """(FtDetectItem array, keepalive) from dicts with stream, occupied [n, 2] float64 pixels (optional) and max_new."""
    arr = (FtDetectItem * max(len(items), 1))()
    keep = []
    for b, d in enumerate(items):
        occ = np.ascontiguousarray(d.get("occupied", np.zeros((0, 2))), dtype=np.float64).reshape(-1, 2)
        keep.append(occ)
        arr[b].stream = int(d.get("stream", 0))
        arr[b].n_occupied = int(d.get("n_occupied", len(occ)))      # n_occupied: for the tests of the argument checks
        arr[b].max_new = int(d["max_new"])
        arr[b].occupied_xy = occ.ctypes.data_as(c_double_p) if len(occ) else None
    return arr, keep


# ---- outlier rejection of the point front end (uvs_ft_reject, include/uvs_solver.h) ---------------------------------------
FT_REJECT_HYPOTHESES = 1000
FT_REJECT_OK, FT_REJECT_SKIPPED, FT_REJECT_NO_MODEL = 0, 1, 2


class FtRejectItem(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("prev_norm", c_double_p), ("next_norm", c_double_p)]


class FtRejectResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_inliers", C.c_int32), ("hypothesis", C.c_int32), ("root", C.c_int32), ("iterations", C.c_int32),
                ("reserved", C.c_int32), ("F", C.c_double * 9)]


def ft_reject_items(items):
    """(FtRejectItem array, keepalive) from dicts with prev [n, 2] and next [n, 2] float64 normalized points and seed."""
    arr = (FtRejectItem * max(len(items), 1))()
    keep = []
    for b, d in enumerate(items):
        prev = np.ascontiguousarray(d["prev"], dtype=np.float64).reshape(-1, 2)
        nxt = np.ascontiguousarray(d["next"], dtype=np.float64).reshape(-1, 2)
        keep += [prev, nxt]
        arr[b].n_points = int(d.get("n_points", len(prev)))          # n_points: for the tests of the argument checks
        arr[b].seed = int(d.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
        arr[b].prev_norm = prev.ctypes.data_as(c_double_p) if len(prev) else None
        arr[b].next_norm = nxt.ctypes.data_as(c_double_p) if len(nxt) else None
    return arr, keep


# ---- equalization of the front ends' images (uvs_ft_set_equalize, uvs_ft_equalize, include/uvs_solver.h) ------------------
FT_CLAHE_MAX_TILES = 16


class FtImage(C.Structure):
    _fields_ = [("image", c_u8_p), ("width", C.c_int32), ("height", C.c_int32)]


def ft_images(images):
    """(FtImage array, keepalive) from [H, W] uint8 arrays."""
    arr = (FtImage * max(len(images), 1))()
    keep = []
    for b, im in enumerate(images):
        im = np.ascontiguousarray(im, dtype=np.uint8)
        keep.append(im)
        arr[b].image = im.ctypes.data_as(c_u8_p)
        arr[b].height, arr[b].width = im.shape
    return arr, keep


# ---- line tracking of the line front end (uvs_lt_*, include/uvs_solver.h) ------------------------------------------------
LT_MAX_STREAMS = 64
LT_MAX_LINES = 1024
LT_MAX_LENGTH = 2048
LT_MIN_SIZE = 8
LT_ROWS = 63
LT_DESC_FLOATS = 72
LT_DESC_BYTES = 32
LT_GATE2 = 900
LT_STATUS = ["OK", "SHORT", "LONG"]      # line_status[] of uvs_lt_track
LT_OK, LT_SHORT, LT_LONG = 0, 1, 2


class LtItem(C.Structure):
    _fields_ = [("image", c_u8_p), ("stream", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_lines", C.c_int32),
                ("segments", c_double_p)]


class LtResult(C.Structure):
    _fields_ = [("n_described", C.c_int32), ("n_matched", C.c_int32), ("status", C.c_int32)]


def lt_items(items):
    """(LtItem array, keepalive) from dicts with stream, image [H, W] uint8 and segs [n, 4] float64 pixels (sx, sy, ex, ey; optional)."""
    arr = (LtItem * max(len(items), 1))()
    keep = []
    for b, d in enumerate(items):
        im = np.ascontiguousarray(d["image"], dtype=np.uint8)
        segs = np.ascontiguousarray(d.get("segs", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4)
        keep += [im, segs]
        arr[b].image = im.ctypes.data_as(c_u8_p)
        arr[b].stream = int(d.get("stream", 0))
        arr[b].height, arr[b].width = im.shape
        arr[b].n_lines = int(d.get("n_lines", len(segs)))            # n_lines: for the tests of the argument checks
        arr[b].segments = segs.ctypes.data_as(c_double_p) if len(segs) else None
    return arr, keep


# ---- segment detection of the line front end (uvs_lt_detect, uvs_lt_detect_track, include/uvs_solver.h) -------------------
LT_DET_MAX_THRESHOLD = 2040
LT_DET_OK, LT_DET_OVERFLOW = 0, 1


class LtDetItem(C.Structure):
    _fields_ = [("image", c_u8_p), ("stream", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32)]


class LtDetParams(C.Structure):
    _fields_ = [("grad_threshold", C.c_int32), ("min_pixels", C.c_int32), ("min_length", C.c_double)]


class LtDetResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_found", C.c_int32), ("n_returned", C.c_int32), ("n_support", C.c_int32), ("n_regions", C.c_int32 * 2)]


def lt_det_items(items):
    """(LtDetItem array, keepalive) from dicts with image [H, W] uint8 and stream (uvs_lt_detect_track's slot; optional)."""
    arr = (LtDetItem * max(len(items), 1))()
    keep = []
    for b, d in enumerate(items):
        im = np.ascontiguousarray(d["image"], dtype=np.uint8)
        keep.append(im)
        arr[b].image = im.ctypes.data_as(c_u8_p)
        arr[b].stream = int(d.get("stream", 0))
        arr[b].height, arr[b].width = im.shape
    return arr, keep


# ---- undistortion of the line front end's images (uvs_lt_set_undistort, uvs_lt_set_remap, uvs_lt_undistort, include/uvs_solver.h) ----
# The camera is a KfCamera (kf_camera), an image of uvs_lt_undistort an LtDetItem (lt_det_items: image and stream), a map int32 [Ho, Wo, 2].
LT_UD_FRACTION_BITS = 5                  # a map word is a position in 1 / 32 px of the raw image
LT_UD_LIMIT = 1 << 24                    # |X|, |Y| of a map word; uvs_lt_set_remap clamps to it

# ---- camera models of the front ends (uvs_camera_model, uvs_ft_set_camera_model, uvs_ft_lift, uvs_lt_set_undistort_model, include/uvs_solver.h) ----
CAM_PINHOLE, CAM_MEI, CAM_KANNALA_BRANDT = 0, 1, 2
CAM_KB_ITERATIONS = 32
# the order of uvs_camera_model.p, and the sections of camodocal's YAML that hold the names
CAM_PARAMS = {CAM_PINHOLE: ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"),
              CAM_MEI: ("xi", "k1", "k2", "p1", "p2", "gamma1", "gamma2", "u0", "v0"),
              CAM_KANNALA_BRANDT: ("k2", "k3", "k4", "k5", "mu", "mv", "u0", "v0")}
CAM_MODEL_TYPES = {"PINHOLE": CAM_PINHOLE, "MEI": CAM_MEI, "KANNALA_BRANDT": CAM_KANNALA_BRANDT}
_CAM_SECTIONS = ("mirror_parameters", "distortion_parameters", "projection_parameters")


class CameraModel(C.Structure):
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("p", C.c_double * 12)]

    def as_tuple(self):
        return int(self.model), tuple(self.p[:len(CAM_PARAMS.get(int(self.model), ()))])


def camera_model(model, params=None):
    """A CameraModel from (model id, parameters in the order of CAM_PARAMS), from a dict of load_camera_calibration, or a CameraModel itself.
    The id is not checked here: the library rejects an unknown one."""
    if isinstance(model, CameraModel):
        return model
    if isinstance(model, dict):
        model, params = model["model"], model["params"]
    m = CameraModel()
    m.model = int(model)
    v = [float(x) for x in params]
    if len(v) > 12:
        raise ValueError("a camera model has at most 12 parameters")
    for i, x in enumerate(v):
        m.p[i] = x
    return m


def load_camera_calibration(path):
    """camodocal's camera YAML (CameraFactory::generateCameraFromYamlFile; the reference's configuration files carry it at their top level) ->
    dict(model: CAM_*, model_type, params: tuple in the order of CAM_PARAMS[model], camera_name, width, height).  The part read is flat OpenCV YAML
    (`key: value` lines and one level of `section:` with indented `key: value` lines), parsed here like load_brief_pattern, without a YAML library."""
    top, sections, section = {}, {}, None
    with open(path) as f:
        for line in f:
            s = line.split("#", 1)[0].rstrip()
            if not s.strip() or s.startswith("%") or s.strip() == "---" or ":" not in s:
                continue
            key, rest = (t.strip() for t in s.split(":", 1))
            if s[0] in " \t":
                if section in _CAM_SECTIONS and rest:
                    sections[section][key] = rest
            else:
                section = key if not rest else None
                if section in _CAM_SECTIONS:
                    sections[section] = {}
                elif rest:
                    top[key] = rest.strip('"')
    kind = top.get("model_type", "").upper()            # (a file without model_type is a pinhole to the reference, too)
    kind = kind or "PINHOLE"
    if kind not in CAM_MODEL_TYPES:
        raise ValueError(f"{path}: model_type {kind!r} is none of {sorted(CAM_MODEL_TYPES)}")
    model = CAM_MODEL_TYPES[kind]
    flat = {}
    for sec in _CAM_SECTIONS:
        flat.update(sections.get(sec, {}))
    try:
        params = tuple(float(flat[k]) for k in CAM_PARAMS[model])
    except (KeyError, ValueError) as e:
        raise ValueError(f"{path}: a {kind} camera needs {', '.join(CAM_PARAMS[model])}") from e
    return dict(model=model, model_type=kind, params=params, camera_name=top.get("camera_name", ""),
                width=int(top.get("image_width", 0)), height=int(top.get("image_height", 0)))

# ---- place recognition of loop closure (uvs_pr_*, include/uvs_solver.h) -------------------------------------------------
PR_MAX_K = 16
PR_MAX_L = 16
PR_MAX_FRAMES = 64
PR_DETECT_RESULTS = 4
PR_HEADER = np.dtype([("k", "<i4"), ("L", "<i4"), ("scoring", "<i4"), ("weighting", "<i4"), ("n_nodes", "<i4"), ("n_words", "<i4")])      # 24 bytes
PR_NODE = np.dtype([("node_id", "<i4"), ("parent_id", "<i4"), ("weight", "<f8"), ("descriptor", "<u8", (4,))])                             # 48 bytes
PR_WORD = np.dtype([("node_id", "<i4"), ("word_id", "<i4")])                                                                               # 8 bytes


def load_vocabulary(path):
    """The reference's binary vocabulary (ThirdParty/VocabularyBinary.hpp: a 24-byte header k, L, scoringType, weightingType, nNodes, nWords;
    nNodes records {int32 nodeId, int32 parentId, double weight, uint64 descriptor[4]}; nWords records {int32 nodeId, int32 wordId}) ->
    dict(k, L, scoring, weighting, node_id, parent_id, weight, descriptor [n, 4] uint64, word_node_id, word_id).  The root is node 0 and has
    no record; descriptor bit i is bit (i & 63) of word (i >> 6)."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < PR_HEADER.itemsize:
        raise ValueError(f"{path}: shorter than the 24-byte header")
    h = np.frombuffer(raw, PR_HEADER, 1)[0]
    nn, nw = int(h["n_nodes"]), int(h["n_words"])
    if nn < 0 or nw < 0 or len(raw) != PR_HEADER.itemsize + nn * PR_NODE.itemsize + nw * PR_WORD.itemsize:
        raise ValueError(f"{path}: {len(raw)} bytes do not hold {nn} node records and {nw} word records")
    nodes = np.frombuffer(raw, PR_NODE, nn, PR_HEADER.itemsize)
    words = np.frombuffer(raw, PR_WORD, nw, PR_HEADER.itemsize + nn * PR_NODE.itemsize)
    return dict(k=int(h["k"]), L=int(h["L"]), scoring=int(h["scoring"]), weighting=int(h["weighting"]),
                node_id=nodes["node_id"].copy(), parent_id=nodes["parent_id"].copy(), weight=nodes["weight"].copy(),
                descriptor=nodes["descriptor"].copy(), word_node_id=words["node_id"].copy(), word_id=words["word_id"].copy())


def save_vocabulary(path, voc):
    """The inverse of load_vocabulary, byte for byte."""
    nodes = np.zeros(len(voc["node_id"]), PR_NODE)
    nodes["node_id"], nodes["parent_id"], nodes["weight"] = voc["node_id"], voc["parent_id"], voc["weight"]
    nodes["descriptor"] = np.asarray(voc["descriptor"], np.uint64).reshape(-1, 4)
    words = np.zeros(len(voc["word_id"]), PR_WORD)
    words["node_id"], words["word_id"] = voc["word_node_id"], voc["word_id"]
    h = np.zeros(1, PR_HEADER)
    h["k"], h["L"], h["scoring"], h["weighting"], h["n_nodes"], h["n_words"] = voc["k"], voc["L"], voc.get("scoring", 0), voc.get("weighting", 0), len(nodes), len(words)
    with open(path, "wb") as f:
        f.write(h.tobytes()); f.write(nodes.tobytes()); f.write(words.tobytes())


def pr_vocabulary_args(voc):
    """(the arguments k .. word_id of uvs_pr_check_vocabulary / uvs_pr_create, keepalive) from a load_vocabulary dict."""
    a = dict(node_id=np.ascontiguousarray(voc["node_id"], np.int32), parent_id=np.ascontiguousarray(voc["parent_id"], np.int32),
             weight=np.ascontiguousarray(voc["weight"], np.float64), descriptor=np.ascontiguousarray(voc["descriptor"], np.uint64).reshape(-1, 4),
             word_node_id=np.ascontiguousarray(voc["word_node_id"], np.int32), word_id=np.ascontiguousarray(voc["word_id"], np.int32))
    if not (len(a["node_id"]) == len(a["parent_id"]) == len(a["weight"]) == len(a["descriptor"])) or len(a["word_node_id"]) != len(a["word_id"]):
        raise ValueError("vocabulary: arrays of unequal length")
    args = [int(voc["k"]), int(voc["L"]), int(voc.get("scoring", 0)), int(voc.get("weighting", 0)), len(a["node_id"]),
            a["node_id"].ctypes.data_as(c_i32_p), a["parent_id"].ctypes.data_as(c_i32_p), _dp(a["weight"]), a["descriptor"].ctypes.data_as(c_u64_p),
            len(a["word_id"]), a["word_node_id"].ctypes.data_as(c_i32_p), a["word_id"].ctypes.data_as(c_i32_p)]
    return args, a


def pr_frames(frames):
    """(n_features int32 [n], descriptors uint64 [sum, 4]) from a list of [n_f, 4] uint64 descriptor arrays (empty ones allowed)."""
    ds = [np.ascontiguousarray(d, dtype=np.uint64).reshape(-1, 4) for d in frames]
    nf = np.array([len(d) for d in ds], np.int32)
    desc = np.ascontiguousarray(np.concatenate(ds) if ds else np.zeros((0, 4), np.uint64))
    if len(desc) == 0:
        desc = np.zeros((1, 4), np.uint64)
    return nf, desc


# ---- triangulation of landmarks (uvs_tri_*, include/uvs_solver.h) ------------------------------------------------
TRI_MAX_WINDOWS = 4096
TRI_MAX_LANDMARKS = 1 << 22
TRI_POINT_FIELDS = ("pt_window", "pt_start", "pt_obs_begin", "pt_obs")
TRI_LINE_FIELDS = ("ln_window", "ln_fi", "ln_fj", "ln_sp_i", "ln_ep_i", "ln_sp_j", "ln_ep_j")


class TriBatch(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("n_points", C.c_int32), ("n_lines", C.c_int32), ("reserved", C.c_int32),
                ("pose", c_double_p), ("ex_pose", c_double_p),
                ("pt_window", c_i32_p), ("pt_start", c_i32_p), ("pt_obs_begin", c_i32_p), ("pt_obs", c_double_p),
                ("ln_window", c_i32_p), ("ln_fi", c_i32_p), ("ln_fj", c_i32_p),
                ("ln_sp_i", c_double_p), ("ln_ep_i", c_double_p), ("ln_sp_j", c_double_p), ("ln_ep_j", c_double_p)]


def tri_batch(batch, null=()):
    """(TriBatch, keepalive) from a dict with the fields of uvs_tri_batch as arrays: pose [n_windows, 11, 7], ex_pose [n_windows, 7] and
    TRI_POINT_FIELDS / TRI_LINE_FIELDS (a kind that is absent or empty passes a count of 0).  `null` names fields passed as NULL."""
    b = TriBatch(); keep = {}
    keep["pose"] = np.ascontiguousarray(batch["pose"], np.float64).reshape(-1, NUM_FRAMES, 7)
    keep["ex_pose"] = np.ascontiguousarray(batch["ex_pose"], np.float64).reshape(-1, 7)
    b.n_windows = len(keep["pose"])
    for name in TRI_POINT_FIELDS + TRI_LINE_FIELDS:
        dt = np.float64 if name in ("pt_obs", "ln_sp_i", "ln_ep_i", "ln_sp_j", "ln_ep_j") else np.int32
        keep[name] = np.ascontiguousarray(batch.get(name, np.zeros(0)), dt)
    b.n_points = len(keep["pt_window"]); b.n_lines = len(keep["ln_window"])
    for name, a in keep.items():
        if name not in null and a.size:
            setattr(b, name, a.ctypes.data_as(c_double_p if a.dtype == np.float64 else c_i32_p))
    return b, keep


# ---- IMU pre-integration for batches of intervals (uvs_imu_*, include/uvs_solver.h) ------------------------------
IMU_MAX_INTERVALS = 65536
IMU_MAX_SAMPLES = 1 << 22
IMU_STAGE_CHUNK = 64
IMU_INTERVAL_FIELDS = ("acc_0", "gyr_0", "ba", "bg")
IMU_SAMPLE_FIELDS = ("dt", "acc", "gyr")
IMU_STATE_FIELDS = ("state_p", "state_R", "state_v")
IMU_BLOCK_DTYPE = np.dtype([("sum_dt", "<f8"), ("delta_p", "<f8", 3), ("delta_q", "<f8", 4), ("delta_v", "<f8", 3), ("linearized_ba", "<f8", 3),
                            ("linearized_bg", "<f8", 3), ("jacobian", "<f8", (15, 15)), ("covariance", "<f8", (15, 15)), ("frame_i", "<i4"), ("skip", "<i4")])
assert IMU_BLOCK_DTYPE.itemsize == C.sizeof(ImuBlock)


class ImuBatch(C.Structure):
    _fields_ = [("n_intervals", C.c_int32), ("sample_begin", c_i32_p), ("acc_0", c_double_p), ("gyr_0", c_double_p), ("ba", c_double_p), ("bg", c_double_p),
                ("frame_i", c_i32_p), ("dt", c_double_p), ("acc", c_double_p), ("gyr", c_double_p),
                ("state_p", c_double_p), ("state_R", c_double_p), ("state_v", c_double_p), ("gravity", C.c_double * 3)]


def imu_batch(batch, null=()):
    """(ImuBatch, keepalive) from a dict with the fields of uvs_imu_batch as arrays: sample_begin [n + 1], IMU_INTERVAL_FIELDS [n, 3],
    IMU_SAMPLE_FIELDS ([m], [m, 3], [m, 3]); optional frame_i [n] and, for the dead reckoning, IMU_STATE_FIELDS ([n, 3], [n, 3, 3], [n, 3])
    with gravity [3].  `null` names fields passed as NULL."""
    b = ImuBatch(); keep = {}
    keep["sample_begin"] = np.ascontiguousarray(batch["sample_begin"], np.int32)
    b.n_intervals = len(keep["sample_begin"]) - 1
    for name in IMU_INTERVAL_FIELDS + IMU_SAMPLE_FIELDS + IMU_STATE_FIELDS:
        if batch.get(name) is not None:
            keep[name] = np.ascontiguousarray(batch[name], np.float64)
    if batch.get("frame_i") is not None:
        keep["frame_i"] = np.ascontiguousarray(batch["frame_i"], np.int32)
    for name, a in list(keep.items()):
        if name not in null:
            p = a if a.size else np.zeros(1, a.dtype)          # an empty array is still a pointer
            keep[name + "_p"] = p
            setattr(b, name, p.ctypes.data_as(c_double_p if a.dtype == np.float64 else c_i32_p))
    g = np.asarray(batch.get("gravity", (0.0, 0.0, 0.0)), np.float64)
    b.gravity[0], b.gravity[1], b.gravity[2] = float(g[0]), float(g[1]), float(g[2])
    return b, keep


def imu_batch_of(intervals, states=None, gravity=None):
    """The batch dict of a list of intervals, each a dict(acc_0, gyr_0, ba, bg, dt [m], acc [m, 3], gyr [m, 3]) with an optional frame_i;
    `states`: per interval (P [3], R [3, 3], V [3]) for the dead reckoning, with `gravity` [3]."""
    n = len(intervals)
    cnt = [len(np.atleast_1d(iv["dt"])) for iv in intervals]
    cat = lambda key, w: (np.concatenate([np.asarray(iv[key], np.float64).reshape(-1, w) for iv in intervals]) if n else np.zeros((0, w)))
    b = dict(sample_begin=np.r_[0, np.cumsum(cnt)].astype(np.int32), dt=cat("dt", 1).reshape(-1), acc=cat("acc", 3), gyr=cat("gyr", 3),
             frame_i=np.array([iv.get("frame_i", 0) for iv in intervals], np.int32))
    for key in IMU_INTERVAL_FIELDS:
        b[key] = np.array([iv[key] for iv in intervals], np.float64).reshape(n, 3)
    if states is not None:
        b["state_p"] = np.array([s[0] for s in states], np.float64).reshape(n, 3)
        b["state_R"] = np.array([s[1] for s in states], np.float64).reshape(n, 3, 3)
        b["state_v"] = np.array([s[2] for s in states], np.float64).reshape(n, 3)
        b["gravity"] = np.asarray(gravity, np.float64)
    return b


# ---- relative pose of window pairs (uvs_rp_*, include/uvs_solver.h) -----------------------------------------------
RP_MAX_ITEMS = 4096
RP_OK, RP_FEW_CORRES, RP_LOW_PARALLAX, RP_FEW_POINTS, RP_NO_MODEL, RP_FEW_INLIERS = range(6)
RP_PARAM_DEFAULTS = dict(focal_length=460.0, min_parallax_px=30.0, f_threshold=0.3 / 460, confidence=0.99, max_depth=50.0, min_corres=20,
                         min_ransac_points=15, min_inliers=12)
RP_ITEM_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("average_parallax", "<f8"),
                                 ("ransac_status", "<i4"), ("n_inliers", "<i4"), ("hypothesis", "<i4"), ("root", "<i4"), ("iterations", "<i4"),
                                 ("ransac_reserved", "<i4"), ("F", "<f8", 9),
                                 ("good", "<i4", 4), ("chosen", "<i4"), ("inlier_cnt", "<i4"), ("ok", "<i4"), ("reserved", "<i4"),
                                 ("R", "<f8", (3, 3)), ("t", "<f8", 3), ("Rotation", "<f8", (3, 3)), ("Translation", "<f8", 3)])
RP_WINDOW_RESULT_DTYPE = np.dtype([("l", "<i4"), ("reserved", "<i4"), ("Rotation", "<f8", (3, 3)), ("Translation", "<f8", 3)])


class RpItem(C.Structure):
    _fields_ = [("window", C.c_int32), ("frame_l", C.c_int32), ("n", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
                ("left", c_double_p), ("right", c_double_p)]


class RpParams(C.Structure):
    _fields_ = [("focal_length", C.c_double), ("min_parallax_px", C.c_double), ("f_threshold", C.c_double), ("confidence", C.c_double),
                ("max_depth", C.c_double), ("min_corres", C.c_int32), ("min_ransac_points", C.c_int32), ("min_inliers", C.c_int32),
                ("reserved", C.c_int32)]


class RpItemResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n", C.c_int32), ("average_parallax", C.c_double), ("ransac", FtRejectResult), ("good", C.c_int32 * 4),
                ("chosen", C.c_int32), ("inlier_cnt", C.c_int32), ("ok", C.c_int32), ("reserved", C.c_int32), ("R", C.c_double * 9),
                ("t", C.c_double * 3), ("Rotation", C.c_double * 9), ("Translation", C.c_double * 3)]


class RpWindowResult(C.Structure):
    _fields_ = [("l", C.c_int32), ("reserved", C.c_int32), ("Rotation", C.c_double * 9), ("Translation", C.c_double * 3)]


assert RP_ITEM_RESULT_DTYPE.itemsize == C.sizeof(RpItemResult) and RP_WINDOW_RESULT_DTYPE.itemsize == C.sizeof(RpWindowResult)


def rp_params(**over):
    """RpParams with the reference's values (RP_PARAM_DEFAULTS), `over` on top."""
    p = RpParams()
    for k, v in {**RP_PARAM_DEFAULTS, **over}.items():
        setattr(p, k, v)
    return p


def rp_items_of(items, null=()):
    """(RpItem array, keepalive) from dicts with window, frame_l, seed and left [n, 2], right [n, 2] float64 normalized points; an optional
    `n` overrides the count passed.  `null` names "left" / "right": passed as NULL in every item."""
    arr = (RpItem * max(len(items), 1))()
    keep = []
    for k, it in enumerate(items):
        l = np.ascontiguousarray(it["left"], np.float64).reshape(-1, 2); r = np.ascontiguousarray(it["right"], np.float64).reshape(-1, 2)
        if len(l) != len(r):
            raise ValueError("rp_items_of: left and right differ in length")
        keep += [l, r]
        arr[k].window = int(it.get("window", 0)); arr[k].frame_l = int(it.get("frame_l", 0)); arr[k].n = int(it.get("n", len(l)))
        arr[k].seed = int(it.get("seed", 0)) & ((1 << 64) - 1)
        if len(l) and "left" not in null:
            arr[k].left = _dp(l)
        if len(r) and "right" not in null:
            arr[k].right = _dp(r)
    return arr, keep
