"""Numpy restatement of the background integrator (csrc/inflx_background.h) and a host build of the real one -- TEST INFRASTRUCTURE.

``Restatement`` integrates one trajectory with the same steppers, error norm and step-size controller as the kernels, in plain
Python floats.  It mirrors csrc/inflx_background.h statement for statement (that is what makes a comparison to 1e-13 possible), so
it checks the C++ against a second spelling of the same algorithm -- it does not check the algorithm itself.  The model comes in
as a callable: ``lambdify`` of ``eom_fields``, V and the kinetic term (``model_functions``), or the host-compiled generated
function (``BackgroundTwin.eom``), which the integrator comparisons use so that they compare the integrators alone.  Independent
checks of the integration are the analytic power-law attractor (``power_law_*``) and scipy's DOP853 (``solve_ivp_reference``).
``BackgroundTwin`` compiles tests/background_twin.cpp -- the generated headers and csrc/inflx_background.h for the CPU.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import math
import os
import subprocess
import tempfile

import numpy as np
import sympy

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_DP = C.POINTER(C.c_double)

COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW = range(5)

# Fehlberg 4(5), the reference's tableau (src/background_solver.rs:232-240)
RKF_A = [
    [],
    [0.25],
    [3.0 / 32.0, 9.0 / 32.0],
    [1932.0 / 2197.0, -7200.0 / 2197.0, 7296.0 / 2197.0],
    [439.0 / 216.0, -8.0, 3680.0 / 513.0, -845.0 / 4104.0],
    [-8.0 / 27.0, 2.0, -3544.0 / 2565.0, 1859.0 / 4104.0, -11.0 / 40.0],
]
RKF_B5 = [16.0 / 135.0, 0.0, 6656.0 / 12825.0, 28561.0 / 56430.0, -9.0 / 50.0, 2.0 / 55.0]
RKF_B4 = [25.0 / 216.0, 0.0, 1408.0 / 2565.0, 2197.0 / 4104.0, -1.0 / 5.0, 0.0]


def model_functions(model, param_slots, modules=("numpy",)):
    """eom(x0, x1, xd0, xd1, p) -> (eom^0, eom^1, V, G_ab xd^a xd^b) from the model's sympy expressions; ``param_slots`` maps a
    parameter's printed name to its ``args[k]`` slot (``CompilationArtifact.symbol_dictionary``)."""
    x0, x1 = model.coordinates
    xd0, xd1 = model.coordinate_tangents
    plain = sympy.printing.c.C99CodePrinter()._print_Symbol
    exprs = [sympy.sympify(e) for e in model.eom_fields] + [sympy.sympify(model.potential)]
    kin = sum(sympy.sympify(model.metric[a][b]) * [xd0, xd1][a] * [xd0, xd1][b] for a in range(2) for b in range(2))
    exprs.append(kin)
    params = sorted({s for e in exprs for s in e.free_symbols} - {x0, x1, xd0, xd1}, key=lambda s: int(param_slots[plain(s)][5:-1]))
    slots = [int(param_slots[plain(s)][5:-1]) for s in params]
    fns = [sympy.lambdify([x0, x1, xd0, xd1, *params], e, modules=list(modules)) for e in exprs]

    def eom(a, b, c, d, p):
        args = [p[k] for k in slots]
        return tuple(float(f(a, b, c, d, *args)) for f in fns)

    return eom


class Restatement:
    """One trajectory, the kernels' algorithm in Python floats."""

    MAX_REJECTIONS = 50
    FIRST_DT = 1e-10

    def __init__(self, eom, p):
        self.eom, self.p = eom, p

    def rhs(self, y):
        e0, e1, V, kin = self.eom(y[0], y[1], y[2], y[3], self.p)
        H = y[4]
        return [y[2], y[3], -e0 - 3.0 * H * y[2], -e1 - 3.0 * H * y[3], V - 3.0 * H * H, H], kin

    def rk4(self, y, f0, h):
        ys = [y[c] + h * (0.5 * f0[c]) for c in range(6)]
        k2, _ = self.rhs(ys)
        ys = [y[c] + h * (0.5 * k2[c]) for c in range(6)]
        k3, _ = self.rhs(ys)
        ys = [y[c] + h * (1.0 * k3[c]) for c in range(6)]
        k4, _ = self.rhs(ys)
        out = []
        for c in range(6):
            acc = (1.0 / 6.0) * f0[c]
            acc += (1.0 / 3.0) * k2[c]
            acc += (1.0 / 3.0) * k3[c]
            acc += (1.0 / 6.0) * k4[c]
            out.append(y[c] + h * acc)
        return out

    def rkf(self, y, f0, h):
        k = [f0]
        for s in range(1, 6):
            ys = []
            for c in range(6):
                acc = RKF_A[s][0] * k[0][c]
                for j in range(1, s):
                    acc += RKF_A[s][j] * k[j][c]
                ys.append(y[c] + h * acc)
            k.append(self.rhs(ys)[0])
        out, e = [], []
        for c in range(6):
            a4, a5 = RKF_B4[0] * k[0][c], RKF_B5[0] * k[0][c]
            for j in range(1, 6):
                a4 += RKF_B4[j] * k[j][c]
                a5 += RKF_B5[j] * k[j][c]
            out.append(y[c] + h * a4)
            e.append(abs(h * a5 - h * a4))
        return out, e

    @staticmethod
    def norm5(e):
        acc = e[0] * e[0]
        for c in range(1, 5):
            acc += e[c] * e[c]
        return math.sqrt(acc)

    def trial(self, method, y, f, h, adaptive):
        if method == "rkf":
            out, e = self.rkf(y, f, h)
            return out, (self.norm5(e) if adaptive else 0.0)
        if not adaptive:
            return self.rk4(y, f, h), 0.0
        big = self.rk4(y, f, h)
        half = self.rk4(y, f, 0.5 * h)
        fh, _ = self.rhs(half)
        out = self.rk4(half, fh, 0.5 * h)
        return out, self.norm5([abs(out[c] - big[c]) for c in range(6)])

    @staticmethod
    def factor(max_err, err):
        if not err > 0.0:
            return 5.0
        q = 0.9 * (max_err / err) ** 0.2
        return min(max(q, 0.2), 5.0)

    def solve(self, init, rows, method="rkf", max_err=1e-6, dt=None, substeps=1, stop_at_end=False):
        """(rows, 7) y[0..5], t; and a dict with status, N_end, last_row, accepted."""
        e0, e1, V, kin = self.eom(init[0], init[1], init[2], init[3], self.p)
        y = [float(init[0]), float(init[1]), float(init[2]), float(init[3]), math.sqrt((V + 0.5 * kin) / 3.0) if V + 0.5 * kin >= 0 else math.nan, 0.0]
        t, h = 0.0, (dt if dt else self.FIRST_DT)
        f, kin = self.rhs(y)
        finite = lambda v: all(math.isfinite(c) for c in v)  # noqa: E731
        status = COMPLETE if finite(y) and finite(f) and math.isfinite(kin) else NONFINITE
        out = np.full((rows, 7), np.nan)
        out[0, :6], out[0, 6] = y, t
        n_end, last_row, accepted = math.nan, 0, 0
        if status == COMPLETE and stop_at_end and 0.5 * kin / (y[4] * y[4]) >= 1.0:  # already past the end of inflation
            status, n_end = ENDED, 0.0
        adaptive = not dt
        for r in range(1, rows):
            st = status
            ended_now = False
            if st == COMPLETE:
                for _ in range(substeps):
                    eps0, n0 = 0.5 * kin / (y[4] * y[4]), y[5]
                    rejections = 0
                    while True:
                        if t + h == t:
                            st = UNDERFLOW
                            break
                        y1, err = self.trial(method, y, f, h, adaptive)
                        ok = finite(y1) and math.isfinite(err)
                        if not adaptive:
                            if not ok:
                                st = NONFINITE
                                break
                            t += h
                            break
                        if ok and err <= 1.1 * max_err:
                            t += h
                            h *= self.factor(max_err, err)
                            break
                        h *= self.factor(max_err, err) if ok else 0.2
                        rejections += 1
                        if rejections >= self.MAX_REJECTIONS:
                            st = REJECTED
                            break
                    if st != COMPLETE:
                        break
                    y = y1
                    accepted += 1
                    f, kin = self.rhs(y)
                    if not (finite(f) and math.isfinite(kin)):
                        st = NONFINITE
                        break
                    if stop_at_end:
                        eps1 = 0.5 * kin / (y[4] * y[4])
                        if eps1 >= 1.0:
                            n_end = n0 + (1.0 - eps0) / (eps1 - eps0) * (y[5] - n0)
                            st = ENDED
                            break
                ended_now = st == ENDED
            valid = st == COMPLETE or ended_now
            if valid:
                last_row = r
                out[r, :6], out[r, 6] = y, t
            status = st
        return out, dict(status=status, N_end=n_end, last_row=last_row, accepted=accepted)


def solve_ivp_reference(eom, p, init, t_end, end_event=False, rtol=1e-12, atol=1e-14):
    """scipy's DOP853 on the same system; with ``end_event`` the integration stops at epsilon_H = 1 and the e-fold count there is returned."""
    from scipy.integrate import solve_ivp

    e0, e1, V, kin = eom(init[0], init[1], init[2], init[3], p)
    y0 = [init[0], init[1], init[2], init[3], math.sqrt((V + 0.5 * kin) / 3.0), 0.0]

    def f(_t, y):
        a, b, V, _k = eom(y[0], y[1], y[2], y[3], p)
        return [y[2], y[3], -a - 3 * y[4] * y[2], -b - 3 * y[4] * y[3], V - 3 * y[4] ** 2, y[4]]

    def event(_t, y):
        return 0.5 * eom(y[0], y[1], y[2], y[3], p)[3] / y[4] ** 2 - 1.0

    event.terminal = True
    event.direction = 1
    sol = solve_ivp(f, (0.0, t_end), y0, method="DOP853", rtol=rtol, atol=atol, events=[event] if end_event else None, dense_output=True)
    return sol


class BackgroundTwin:
    """tests/background_twin.cpp built for the CPU from an artefact's generated headers (contraction off: the twin's arithmetic is the
    restatement's, operation for operation)."""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        """``contract="fast"`` lets the compiler fuse a*b+c into FMAs (the CPU must have them), as hipcc does for the kernels."""
        header_text = artifact._build[0]
        eom_text = artifact.eom_header_text()
        background_h = open(os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_background.h")).read()
        twin_cpp = open(os.path.join(HERE, "background_twin.cpp")).read()
        tag = hashlib.sha1((header_text + eom_text + background_h + twin_cpp + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_background_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".so"))
        if not os.path.exists(so):
            for path, text in ((hdr, header_text), (eom_hdr, eom_text)):
                with open(path, "w") as fh:
                    fh.write(text)
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas",
                f"-I{os.path.join(ROOT, 'inflatox_amd', 'csrc')}", f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"',
                os.path.join(HERE, "background_twin.cpp"), "-o", so + ".tmp",
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(so + ".tmp", so)
        self.lib = C.CDLL(so)
        self.lib.twin_eom.argtypes = [_DP, _DP, C.c_size_t, _DP]
        self.lib.twin_solve.argtypes = [_DP, _DP, C.c_size_t, C.c_uint, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP]
        self.lib.twin_sf_status_take.restype = C.c_uint

    def sf_status_take(self) -> int:
        """The bits (csrc/inflx_sf.h: INFLX_SF_EDOM = 1, INFLX_SF_EDECLINED = 2) the model's special functions have set in this build
        since they were last read; reading clears them."""
        return int(self.lib.twin_sf_status_take())

    def eom(self, p, pts):
        p = np.ascontiguousarray(p, dtype=np.float64)
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        out = np.empty((pts.shape[0], 4))
        self.lib.twin_eom(p.ctypes.data_as(_DP), pts.ctypes.data_as(_DP), pts.shape[0], out.ctypes.data_as(_DP))
        return out

    def solve(self, p, init, rows, method="rkf", max_err=1e-6, dt=None, substeps=1, stop_at_end=False):
        p = np.ascontiguousarray(p, dtype=np.float64)
        init = np.ascontiguousarray(init, dtype=np.float64)
        out = np.empty((rows, 7))
        meta = np.empty(4)
        self.lib.twin_solve(p.ctypes.data_as(_DP), init.ctypes.data_as(_DP), rows, substeps, 1 if method == "rkf" else 0, max_err, dt or 0.0,
                            int(stop_at_end), out.ctypes.data_as(_DP), meta.ctypes.data_as(_DP))  # fmt: skip
        return out, dict(status=int(meta[0]), N_end=meta[1], last_row=int(meta[2]), accepted=int(meta[3]))


# ---- the analytic power-law attractor: V = V0 exp(-lam phi) on a flat field space ---------------------------------------------
LAM, V0 = 0.5, 1.0
P_POW = 2.0 / LAM**2  # p = 8: a ~ t^p


def power_law_model():
    from inflatox_amd import InflationModelBuilder

    phi, theta, v0, lam = sympy.symbols("phi theta V0 lam")
    return InflationModelBuilder.new([phi, theta], [[1, 0], [0, 1]], v0 * sympy.exp(-lam * phi), model_name="power_law", init_sympy_printing=False, silent=True).build()


def power_law_artifact():
    from inflatox_amd import Compiler

    art = Compiler(power_law_model(), silent=True).compile()
    p = np.zeros(art.n_parameters)
    p[int(art.symbol_dictionary["V0"][5:-1])] = V0
    p[int(art.symbol_dictionary["lam"][5:-1])] = LAM
    return art, p


# ---- a potential with a wall: V = V0 + m phi^(3/2) on a flat field space, finite at phi = 0 (V = V0, dV = 0), NaN for every phi < 0 --
WALL_V0, WALL_M = 1.0, 1.0


def wall_model():
    from inflatox_amd import InflationModelBuilder

    phi, theta, v0, m = sympy.symbols("phi theta V0 m")
    return InflationModelBuilder.new([phi, theta], [[1, 0], [0, 1]], v0 + m * phi ** sympy.Rational(3, 2), model_name="wall", init_sympy_printing=False, silent=True).build()


def wall_artifact():
    from inflatox_amd import Compiler

    art = Compiler(wall_model(), silent=True).compile()
    p = np.zeros(art.n_parameters)
    p[int(art.symbol_dictionary["V0"][5:-1])] = WALL_V0
    p[int(art.symbol_dictionary["m"][5:-1])] = WALL_M
    return art, p


def power_law_init():
    """(phi, theta, phidot, thetadot) at t = 1 on the attractor: phidot = 2/lam, H = p, V = p(3p - 1)."""
    return np.array([-math.log(P_POW * (3 * P_POW - 1) / V0) / LAM, 0.0, 2.0 / LAM, 0.0])


def power_law_exact(t):
    """(phi, theta, phidot, thetadot, H, N) at integration time t (cosmic time 1 + t)."""
    tt = 1.0 + np.asarray(t, dtype=np.float64)
    phi1 = power_law_init()[0]
    return np.stack([phi1 + (2.0 / LAM) * np.log(tt), 0 * tt, 2.0 / (LAM * tt), 0 * tt, P_POW / tt, P_POW * np.log(tt)], axis=-1)
