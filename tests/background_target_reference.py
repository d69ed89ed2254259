"""Host build of the target-on-N stepper (csrc/inflx_background.h: inflx_bg_step_target) and a numpy spelling of its dense output
-- TEST INFRASTRUCTURE.

``TargetTwin`` compiles tests/background_target_twin.cpp the way ``background_reference.BackgroundTwin`` compiles its twin: the
artefact's generated headers and csrc/inflx_background.h for the CPU, contraction off.  ``hermite`` is the cubic Hermite
interpolant over one accepted step, written independently of the C++ (polynomial in theta, not in the basis functions).
"""

from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_DP = C.POINTER(C.c_double)

TARGET = 5


class TargetTwin:
    """tests/background_target_twin.cpp built for the CPU from an artefact's generated headers."""

    def __init__(self, artifact, cxx: str = "g++"):
        header_text = artifact._build[0]
        eom_text = artifact.eom_header_text()
        sources = [os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_background.h"), os.path.join(HERE, "background_target_twin.cpp")]
        tag = hashlib.sha1((header_text + eom_text + "".join(open(f).read() for f in sources)).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_background_target_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".so"))
        if not os.path.exists(so):
            for path, text in ((hdr, header_text), (eom_hdr, eom_text)):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas",
                f"-I{os.path.join(ROOT, 'inflatox_amd', 'csrc')}", f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"',
                sources[1], "-o", tmp,
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_solve_target.argtypes = [_DP, _DP, C.c_double, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP]
        self.lib.twin_solve_target.restype = None

    def solve(self, p, init, target, max_steps, method="rkf", max_err=1e-8, dt=None, stop_at_end=False):
        """(out (8): y[0..5], t, epsilon_H where the lane stopped; dict with status, N_end, accepted)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        init = np.ascontiguousarray(init, dtype=np.float64)
        out = np.empty(8)
        meta = np.empty(3)
        self.lib.twin_solve_target(p.ctypes.data_as(_DP), init.ctypes.data_as(_DP), float(target), int(max_steps), 1 if method == "rkf" else 0,
                                   max_err, dt or 0.0, int(stop_at_end), out.ctypes.data_as(_DP), meta.ctypes.data_as(_DP))  # fmt: skip
        return out, dict(status=int(meta[0]), N_end=meta[1], accepted=int(meta[2]))


def rhs(eom_row, y):
    """dy/dt of the six-component state from one row (eom^0, eom^1, V, kin) of the model function at it."""
    e0, e1, V, _ = eom_row
    H = y[4]
    return np.array([y[2], y[3], -e0 - 3.0 * H * y[2], -e1 - 3.0 * H * y[3], V - 3.0 * H * H, H])


def hermite(y0, f0, y1, f1, h, theta):
    """The cubic through (0, y0) and (1, y1) with slopes h f0 and h f1, as a polynomial in theta."""
    d = y1 - y0
    a, b = h * f0, h * f1
    return y0 + theta * (a + theta * ((3.0 * d - 2.0 * a - b) + theta * (a + b - 2.0 * d)))


def hermite_state_at(y0, f0, y1, f1, h, n_target):
    """(theta, six-component state) where the interpolant's N equals n_target: the real root in [0, 1] of the cubic, by numpy.roots."""
    d = y1[5] - y0[5]
    a, b = h * f0[5], h * f1[5]
    roots = np.roots([a + b - 2.0 * d, 3.0 * d - 2.0 * a - b, a, y0[5] - n_target])
    real = roots[np.abs(roots.imag) < 1e-12].real
    inside = real[(real >= -1e-12) & (real <= 1.0 + 1e-12)]
    assert inside.size == 1, roots
    theta = float(np.clip(inside[0], 0.0, 1.0))
    y = hermite(y0, f0, y1, f1, h, theta)
    y[5] = n_target
    return theta, y
