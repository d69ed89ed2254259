"""Host build of the sampled stepper (csrc/inflx_background.h: inflx_bg_init_sampled, inflx_bg_step_sampled) -- TEST INFRASTRUCTURE.

``SampledTwin`` compiles tests/background_sampled_twin.cpp the way ``background_target_reference.TargetTwin`` compiles its twin: the
artefact's generated headers and csrc/inflx_background.h for the CPU, contraction off.
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

# EGNO against the host build within RESTATEMENT_TOL["egno"] (test_background_gpu.py): that bound was measured on one trajectory and
# holds where the model is well conditioned.  EGNO's eom^a cancel to ~1e-7 at some points (test_background.py), and a trajectory
# that passes one carries the rounding of an FMA on: of initial_state("egno", seed) for seed < 200 the host build itself, compiled
# with and without contraction, differs by more than the bound (1e-12) for a third of them after 50 steps of 1e-3, by up to 2e-7.
# These are the first 64 seeds for which the two host builds agree within 5e-14, rk4 and rkf, at the samples HEAVY_SAMPLES:
# 1e-13, which test_background_sampled.py asserts, is a tenth of the bound, the factor that RESTATEMENT_TOL leaves.
HEAVY_SAMPLES = (0.0, 0.0105, 0.025, 0.0495)
EGNO_SEEDS = (
    4, 9, 10, 13, 14, 15, 17, 21, 28, 31, 37, 41, 42, 45, 46, 51, 55, 56, 57, 62, 64, 66, 72, 74, 76, 77, 79, 82, 84, 86, 92, 93,
    96, 98, 100, 101, 104, 106, 108, 109, 110, 114, 117, 118, 119, 120, 121, 122, 123, 124, 125, 128, 133, 134, 137, 140, 141, 144, 146, 147, 148, 153, 158, 159,
)  # fmt: skip


class SampledTwin:
    """tests/background_sampled_twin.cpp built for the CPU from an artefact's generated headers."""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        """``contract="fast"`` lets the compiler fuse a*b+c into FMAs (the CPU must have them), as hipcc does for the kernels: the two
        builds differ by that rounding alone, which measures how far a trajectory carries it (``EGNO_SEEDS``)."""
        header_text = artifact._build[0]
        eom_text = artifact.eom_header_text()
        sources = [os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_background.h"), os.path.join(HERE, "background_sampled_twin.cpp")]
        tag = hashlib.sha1((header_text + eom_text + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_background_sampled_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".so"))
        if not os.path.exists(so):
            for path, text in ((hdr, header_text), (eom_hdr, eom_text)):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas",
                f"-I{os.path.join(ROOT, 'inflatox_amd', 'csrc')}", f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"',
                sources[1], "-o", tmp,
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_solve_sampled.argtypes = [_DP, _DP, _DP, C.c_uint, C.c_int, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP, _DP]
        self.lib.twin_solve_sampled.restype = None

    def solve(self, p, init, samples, max_steps, method="rkf", max_err=1e-8, dt=None, stop_at_end=False, at="N"):
        """(out (S, 8): y[0..5], t, epsilon_H at every sample, NaN where not emitted; dict with status, N_end, accepted, n_stored and
        step_of (S): the accepted step that emitted each sample, 0 = init)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        init = np.ascontiguousarray(init, dtype=np.float64)
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        out = np.empty((samples.size, 8))
        step_of = np.empty(samples.size)
        meta = np.empty(4)
        self.lib.twin_solve_sampled(p.ctypes.data_as(_DP), init.ctypes.data_as(_DP), samples.ctypes.data_as(_DP), samples.size, int(at == "t"),
                                    int(max_steps), 1 if method == "rkf" else 0, max_err, dt or 0.0, int(stop_at_end), out.ctypes.data_as(_DP),
                                    step_of.ctypes.data_as(_DP), meta.ctypes.data_as(_DP))  # fmt: skip
        return out, dict(status=int(meta[0]), N_end=meta[1], accepted=int(meta[2]), n_stored=int(meta[3]), step_of=step_of)
