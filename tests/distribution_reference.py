"""Host twin of the first-passage histograms (csrc/inflx_distribution.h) and the bin rule in numpy -- TEST INFRASTRUCTURE.

* ``bin_samples`` applies the stated rule to samples and statuses: k = floor((N - lo) * (bins / (hi - lo))), N < lo below, k >= bins
  above, over the realisations that ENDED; and ``bincount`` of the statuses.  Every expected histogram of the tests is this function on
  the samples of ``stochastic_efolds`` / ``StochasticTwin``.
* ``DistributionTwin`` compiles tests/distribution_twin.cpp -- the generated headers and the code the kernels run -- for the CPU and
  runs the L lanes of every point serially with a shared ticket, in any order of the lanes.
* ``chi2_two_samples`` is the two-sample chi-squared statistic of two histograms after neighbouring bins have been merged until
  every merged bin holds at least ``least`` pooled counts.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from stochastic_reference import CSRC, ENDED, HERE, StochasticTwin

_DP = C.POINTER(C.c_double)
_UP = C.POINTER(C.c_uint32)


def bin_samples(N, status, lo, hi, bins):
    """(row (bins + 2,) int64: below, bins, above of N[status == ENDED]; counts (6,) of the statuses) by the stated rule"""
    N, status = np.asarray(N, dtype=np.float64).reshape(-1), np.asarray(status).reshape(-1).astype(np.int64)
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(bins) / (hi - lo)
    n = N[status == ENDED]
    k = np.floor((n - lo) * scale)
    below = (n < lo) | (k < 0)
    above = ~below & (k >= bins)
    inside = ~below & ~above
    row = np.zeros(bins + 2, dtype=np.int64)
    row[0], row[-1] = below.sum(), above.sum()
    row[1:-1] = np.bincount(k[inside].astype(np.int64), minlength=bins)
    return row, np.bincount(status, minlength=6)


class TwinDistribution:
    """hist (B, bins), below, above (B,), counts (B, 6), launches"""

    def __init__(self, rows, counts, launches):
        self.rows, self.hist, self.below, self.above = rows, rows[:, 1:-1], rows[:, 0], rows[:, -1]
        self.counts, self.launches = counts, launches


class DistributionTwin:
    """tests/distribution_twin.cpp built for the CPU from an artefact's generated headers, contraction off like the other twins"""

    def __init__(self, artifact, cxx: str = "g++"):
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.noise_header_text())
        sources = [os.path.join(CSRC, f) for f in ("inflx_background.h", "inflx_stochastic.h", "inflx_philox.h", "inflx_distribution.h")]
        sources.append(os.path.join(HERE, "distribution_twin.cpp"))
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources)).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_distribution_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, noise_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".noise.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr, noise_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            subprocess.run([cxx, "-O2", "-fPIC", "-shared", "-o", tmp, *StochasticTwin.compile_options(hdr, eom_hdr, noise_hdr), sources[-1]], check=True)
            os.replace(tmp, so)
        self.headers = (hdr, eom_hdr, noise_hdr)
        self.source = sources[-1]
        self.lib = lib = C.CDLL(so)
        lib.twin_slots.argtypes = [_DP, C.c_size_t, C.c_double, C.c_double, C.c_uint32, _UP]
        lib.twin_slots.restype = None
        lib.twin_distribution.argtypes = [_DP, C.c_size_t, _DP, C.c_size_t, C.c_uint64, C.c_uint64, C.c_size_t, _UP, C.c_uint64, C.c_double, C.c_double, C.c_uint64,
                                          C.c_int, C.c_double, C.c_double, C.c_uint32, _DP, C.c_uint32, _UP, C.c_long, _UP, _UP]  # fmt: skip
        lib.twin_distribution.restype = C.c_long

    def slots(self, values, lo, hi, bins):
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.empty(v.size, dtype=np.uint32)
        self.lib.twin_slots(v.ctypes.data_as(_DP), v.size, lo, np.float64(bins) / (np.float64(hi) - np.float64(lo)), bins, out.ctypes.data_as(_UP))
        return out

    def run(self, pars, init, R, bins, N_range, *, lanes_per_point=64, first_realisation=0, streams=None, seed=0, noise_scale=1.0, dN_max=1.0 / 32.0,
            max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, window=256, order=None, launch_limit=None) -> TwinDistribution:  # fmt: skip
        init = np.ascontiguousarray(init, dtype=np.float64).reshape(-1, 4)
        B, L = init.shape[0], lanes_per_point
        p = np.ascontiguousarray(pars, dtype=np.float64)
        ids = np.ascontiguousarray(np.arange(B) if streams is None else streams, dtype=np.uint32)
        r = np.broadcast_to(np.asarray(N_range, dtype=np.float64).reshape(-1, 2), (B, 2))
        bin_ = np.ascontiguousarray(np.stack([r[:, 0], np.float64(bins) / (r[:, 1] - r[:, 0])], axis=1))
        order = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
        assert order is None or sorted(order.tolist()) == list(range(L))
        if launch_limit is None:
            # the bound of inflx_stochastic_distribution (include/inflx_hip_distribution.h) at this window
            first = min(L, R)
            launch_limit = (-(-R // first) + 1) * (-(-max_steps // window) + 1) + 2
        rows, counts = np.empty((B, bins + 2), dtype=np.uint32), np.empty((B, 6), dtype=np.uint32)
        launches = self.lib.twin_distribution(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), B, R, first_realisation, L,
                                              ids.ctypes.data_as(_UP), seed, noise_scale, dN_max, max_steps, 1 if solver == "rkf" else 0, max_err, dt or 0.0, bins,
                                              bin_.ctypes.data_as(_DP), window, None if order is None else order.ctypes.data_as(_UP), launch_limit,
                                              rows.ctypes.data_as(_UP), counts.ctypes.data_as(_UP))  # fmt: skip
        assert launches >= 0, f"the twin went past {launch_limit} launches"
        return TwinDistribution(rows.astype(np.int64), counts.astype(np.int64), launches)


def chi2_two_samples(a, b, least=40):
    """(chi2, dof) of two rows of counts (below, bins, above) after merging neighbours, from the left, until every merged bin holds at
    least ``least`` pooled counts (the last merged bin takes what is left): sum (sqrt(nb / na) a_k - sqrt(na / nb) b_k)^2 / (a_k + b_k),
    dof = merged bins - 1"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ma, mb, sa, sb = [], [], 0.0, 0.0
    for x, y in zip(a, b):
        sa, sb = sa + x, sb + y
        if sa + sb >= least:
            ma.append(sa)
            mb.append(sb)
            sa = sb = 0.0
    if sa + sb > 0.0:
        if ma:
            ma[-1] += sa
            mb[-1] += sb
        else:
            ma.append(sa)
            mb.append(sb)
    ma, mb = np.array(ma), np.array(mb)
    na, nb = ma.sum(), mb.sum()
    chi2 = float((((nb / na) ** 0.5 * ma - (na / nb) ** 0.5 * mb) ** 2 / (ma + mb)).sum())
    return chi2, len(ma) - 1
