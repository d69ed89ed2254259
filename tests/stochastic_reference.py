"""Numpy restatement and host twin of the stochastic e-folds (csrc/inflx_stochastic.h, csrc/inflx_philox.h) -- TEST INFRASTRUCTURE.

* ``philox4x32_10``, ``uniform`` and ``normals`` restate the random numbers in uint64 arithmetic, vectorised over counters.
* ``noise_functions`` derives the factor e of the inverse metric (a Cholesky factor of ``G.inv()``) and Gamma^a = G^bc Gamma^a_bc (the
  connection from the inverse metric, as a textbook writes it) from the sympy model; ``model_functions`` is
  ``background_reference.model_functions`` with numpy: the restatement's model never passes through the transpiler.
* ``StochasticRestatement`` is the stepper of ``background_reference.Restatement`` restated once more over arrays of lanes -- the same
  operations in the same order, every lane with its own step control -- with the kick, the bound on dN, the stop on N and the statuses
  of csrc/inflx_stochastic.h.  Its normals come from ``normals`` (the same stream as the kernels': lane-by-lane comparisons) or from
  ``numpy.random.default_rng`` (an independent stream: comparisons in law).
* ``StochasticTwin`` compiles tests/stochastic_twin.cpp -- the generated headers and the code the kernels run -- for the CPU.

``python tests/stochastic_reference.py`` measures the twin's difference with and without FMA contraction and writes it into
profiles/background_stochastic.json (``d``); ``bound`` is what the lane-by-lane tests assert: 1e-10 + 2 d.
"""

from __future__ import annotations

import ctypes as C
import functools
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
PROFILE = os.path.join(ROOT, "profiles", "background_stochastic.json")
_DP = C.POINTER(C.c_double)
_UP = C.POINTER(C.c_uint32)

RUNNING, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5
COMPLETE = RUNNING
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586476925286766559


# ---- the random numbers --------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) -- arrays or numbers -- under the key (k0, k1): four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniform(hi, lo):
    """u in (0, 1): ((hi << 20 | lo >> 12) + 1/2) 2^-52"""
    k = (np.asarray(hi, dtype=np.uint64) << np.uint64(20)) | (np.asarray(lo, dtype=np.uint64) >> np.uint64(12))
    return (k.astype(np.float64) + 0.5) * 2.0**-52


def normals(seed, step, r, stream):
    """(xi0, xi1) of the counters (step low, step high, r, stream) under the key ``seed``"""
    step = np.asarray(step, dtype=np.uint64)
    w = philox4x32_10(step & MASK, step >> np.uint64(32), r, stream, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = uniform(w[0], w[1]), uniform(w[2], w[3])
    rad, ang = np.sqrt(-2.0 * np.log(u1)), TWO_PI * u2
    return rad * np.cos(ang), rad * np.sin(ang)


# ---- the model, from sympy -----------------------------------------------------------------------------------------------------------
def _slots(model, param_slots, exprs):
    plain = sp.printing.c.C99CodePrinter()._print_Symbol
    free = set().union(*[sp.sympify(e).free_symbols for e in exprs]) - set(model.coordinates) - set(model.coordinate_tangents)
    params = sorted(free, key=lambda s: int(param_slots[plain(s)][5:-1]))
    return params, [int(param_slots[plain(s)][5:-1]) for s in params]


def _vector_function(symbols, exprs, slots):
    fn = sp.lambdify(symbols, [sp.sympify(e) for e in exprs], modules="numpy", cse=True)

    def f(*args_p):
        *args, p = args_p
        with np.errstate(all="ignore"):
            vals = fn(*args, *[p[k] for k in slots])
        shape = np.broadcast(*args).shape
        return [np.broadcast_to(np.asarray(v, dtype=np.float64), shape) for v in vals]

    return f


def model_functions(model, param_slots):
    """eom(x0, x1, xd0, xd1, p) -> [eom^0, eom^1, V, G_ab xd^a xd^b] over arrays of lanes"""
    x = list(model.coordinates)
    xd = list(model.coordinate_tangents)
    kin = sum(sp.sympify(model.metric[a][b]) * xd[a] * xd[b] for a in range(2) for b in range(2))
    exprs = [*model.eom_fields, model.potential, kin]
    params, slots = _slots(model, param_slots, exprs)
    return _vector_function([*x, *xd, *params], exprs, slots)


def noise_expressions(model):
    """(e (2 x 2, lower triangular, e e^T = G^-1), [Gamma^0, Gamma^1]) in sympy: the factor is the Cholesky factor of the inverse
    metric, the connection is written with the inverse metric -- neither is how staging.emit_noise_header derives them"""
    X = list(model.coordinates)
    G = sp.Matrix(2, 2, lambda a, b: sp.sympify(model.metric[a][b]))
    Gi = G.inv()
    e00 = sp.sqrt(Gi[0, 0])
    e10 = Gi[1, 0] / e00
    e11 = sp.sqrt(Gi[1, 1] - e10**2)
    gam = [sum(Gi[b, c] * sum(Gi[a, d] * (sp.diff(G[d, b], X[c]) + sp.diff(G[d, c], X[b]) - sp.diff(G[b, c], X[d])) for d in range(2)) / 2
               for b in range(2) for c in range(2)) for a in range(2)]  # fmt: skip
    return sp.Matrix([[e00, 0], [e10, e11]]), gam, Gi


def noise_functions(model, param_slots):
    """noise(x0, x1, p) -> [e00, e10, e11, Gamma^0, Gamma^1] over arrays of lanes"""
    e, gam, _gi = noise_expressions(model)
    exprs = [e[0, 0], e[1, 0], e[1, 1], *gam]
    params, slots = _slots(model, param_slots, exprs)
    return _vector_function([*model.coordinates, *params], exprs, slots)


# ---- the stepper, over arrays of lanes ---------------------------------------------------------------------------------------------------
from background_reference import RKF_A, RKF_B4, RKF_B5  # noqa: E402

MAX_REJECTIONS, FIRST_DT, MAX_LOCATE = 50, 1e-10, 64


def _hermite(y0, f0, y1, f1, h, th):
    u = 1.0 - th
    h00, h10, h01, h11 = (1.0 + 2.0 * th) * u * u, th * u * u, th * th * (3.0 - 2.0 * th), -(th * th) * u
    return h00 * y0 + h10 * (h * f0) + h01 * y1 + h11 * (h * f1)


def _hermite_slope(y0, f0, y1, f1, h, th):
    u = 1.0 - th
    d00, d10, d11 = -6.0 * th * u, u * (1.0 - 3.0 * th), th * (3.0 * th - 2.0)
    return d00 * y0 + d10 * (h * f0) - d00 * y1 + d11 * (h * f1)


def _locate(n0, h0, n1, h1, h, target):
    """csrc/inflx_background.h inflx_bg_locate over arrays"""
    lo, hi = np.zeros_like(n0), np.ones_like(n0)
    with np.errstate(all="ignore"):
        th = (target - n0) / (n1 - n0)
    th = np.where(th > 0.0, th, 0.0)
    th = np.where(th > 1.0, 1.0, th)
    live = np.ones(n0.shape, dtype=bool)
    for _ in range(MAX_LOCATE):
        g = _hermite(n0, h0, n1, h1, h, th) - target
        live = live & (g != 0.0)
        if not live.any():
            break
        lo = np.where(live & (g < 0.0), th, lo)
        hi = np.where(live & ~(g < 0.0), th, hi)
        with np.errstate(all="ignore"):
            nxt = th - g / _hermite_slope(n0, h0, n1, h1, h, th)
        nxt = np.where((nxt > lo) & (nxt < hi), nxt, 0.5 * (lo + hi))
        moved = np.abs(nxt - th)
        th = np.where(live, nxt, th)
        live = live & ~((moved <= 1e-15) | (hi - lo <= 1e-15))
    return th


class StochasticResult:
    """N (n,): N_end of an ENDED lane, the e-fold count where it stopped otherwise; state (n, 5); status (n,); accepted (n,): the step
    indices a lane went through; by_kick (n,): the lane ended because epsilon_H >= 1 after a kick"""

    def __init__(self, N, state, status, accepted, by_kick):
        self.N, self.state, self.status, self.accepted, self.by_kick = N, state, status, accepted, by_kick


class StochasticRestatement:
    """csrc/inflx_stochastic.h over arrays of lanes; ``eom`` and ``noise`` from ``model_functions`` / ``noise_functions``"""

    def __init__(self, eom, noise, p):
        self.eom, self.noise, self.p = eom, noise, np.asarray(p, dtype=np.float64)

    def rhs(self, y):
        e0, e1, V, kin = self.eom(y[0], y[1], y[2], y[3], self.p)
        return self.rhs_from(y, (e0, e1, V, kin)), kin

    @staticmethod
    def rhs_from(y, o):
        H = y[4]
        return [y[2], y[3], -o[0] - 3.0 * H * y[2], -o[1] - 3.0 * H * y[3], o[2] - 3.0 * H * H, H]

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
            acc = acc + (1.0 / 3.0) * k2[c]
            acc = acc + (1.0 / 3.0) * k3[c]
            acc = acc + (1.0 / 6.0) * k4[c]
            out.append(y[c] + h * acc)
        return out

    def rkf(self, y, f0, h):
        k = [f0]
        for s in range(1, 6):
            ys = []
            for c in range(6):
                acc = RKF_A[s][0] * k[0][c]
                for j in range(1, s):
                    acc = acc + RKF_A[s][j] * k[j][c]
                ys.append(y[c] + h * acc)
            k.append(self.rhs(ys)[0])
        out, e = [], []
        for c in range(6):
            a4, a5 = RKF_B4[0] * k[0][c], RKF_B5[0] * k[0][c]
            for j in range(1, 6):
                a4 = a4 + RKF_B4[j] * k[j][c]
                a5 = a5 + RKF_B5[j] * k[j][c]
            out.append(y[c] + h * a4)
            e.append(np.abs(h * a5 - h * a4))
        return out, e

    @staticmethod
    def norm5(e):
        acc = e[0] * e[0]
        for c in range(1, 5):
            acc = acc + e[c] * e[c]
        return np.sqrt(acc)

    def trial(self, method, y, f, h, adaptive):
        if method == "rkf":
            out, e = self.rkf(y, f, h)
            return out, (self.norm5(e) if adaptive else np.zeros_like(h))
        if not adaptive:
            return self.rk4(y, f, h), np.zeros_like(h)
        big = self.rk4(y, f, h)
        half = self.rk4(y, f, 0.5 * h)
        fh, _ = self.rhs(half)
        out = self.rk4(half, fh, 0.5 * h)
        return out, self.norm5([np.abs(out[c] - big[c]) for c in range(6)])

    @staticmethod
    def factor(max_err, err):
        with np.errstate(all="ignore"):
            q = 0.9 * (max_err / err) ** 0.2
        q = np.where(q < 0.2, 0.2, np.where(q > 5.0, 5.0, q))
        return np.where(err > 0.0, q, 5.0)

    def run(self, init, R, *, streams=None, seed=0, noise_scale=1.0, dN_max=1.0 / 32.0, N_stop=None, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None,
            rng=None) -> StochasticResult:  # fmt: skip
        """B points ``init`` (B, 4) x R realisations, lane = b R + r.  ``rng``: a ``numpy.random.Generator`` to draw the normals from
        in place of Philox."""
        init = np.asarray(init, dtype=np.float64).reshape(-1, 4)
        B = init.shape[0]
        n = B * R
        stream = np.repeat(np.arange(B, dtype=np.uint64) if streams is None else np.asarray(streams, dtype=np.uint64), R)
        real = np.tile(np.arange(R, dtype=np.uint64), B)
        start = np.repeat(init, R, axis=0)
        with np.errstate(all="ignore"):
            _e0, _e1, V, kin = self.eom(start[:, 0], start[:, 1], start[:, 2], start[:, 3], self.p)
            y = [start[:, 0].copy(), start[:, 1].copy(), start[:, 2].copy(), start[:, 3].copy(), np.sqrt((V + 0.5 * kin) / 3.0), np.zeros(n)]
            f, kin = self.rhs(y)
        f, kin = [np.array(c) for c in f], np.array(kin)
        finite = lambda v: np.all(np.isfinite(np.stack(v)), axis=0)  # noqa: E731
        status = np.where(finite(y) & finite(f) & np.isfinite(kin), RUNNING, NONFINITE)
        n_end = np.full(n, np.nan)
        with np.errstate(all="ignore"):
            past = (status == RUNNING) & (0.5 * kin / (y[4] * y[4]) >= 1.0)
        status[past], n_end[past] = ENDED, 0.0
        t, h = np.zeros(n), np.full(n, dt if dt else FIRST_DT)
        accepted, by_kick = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
        adaptive, n_stop = not dt, (math.nan if N_stop is None else float(N_stop))
        for step in range(max_steps):
            idx = np.flatnonzero(status == RUNNING)
            if idx.size == 0:
                break
            accepted[idx] += 1
            with np.errstate(all="ignore"):
                self._step(idx, step, y, f, kin, t, h, status, n_end, by_kick, adaptive, max_err, solver, dN_max, n_stop, noise_scale, seed, real, stream, rng)
        N = np.where(status == ENDED, n_end, y[5])
        return StochasticResult(N, np.stack(y[:5], axis=1), status, accepted, by_kick)

    def _step(self, idx, step, y, f, kin, t, h, status, n_end, by_kick, adaptive, max_err, solver, dN_max, n_stop, noise_scale, seed, real, stream, rng):
        ya, fa, kina = [c[idx] for c in y], [c[idx] for c in f], kin[idx]
        ta, ha = t[idx], h[idx]
        if adaptive:
            cap = dN_max / ya[4]
            ha = np.where((cap > 0.0) & (ha > cap), cap, ha)
        eps0, n0 = 0.5 * kina / (ya[4] * ya[4]), ya[5]
        st = np.full(idx.size, RUNNING)
        y1 = [c.copy() for c in ya]
        taken = ha.copy()
        todo = np.arange(idx.size)
        rejections = np.zeros(idx.size, dtype=np.int64)
        while todo.size:
            under = ta[todo] + ha[todo] == ta[todo]
            st[todo[under]] = UNDERFLOW
            todo = todo[~under]
            if not todo.size:
                break
            out, err = self.trial(solver, [c[todo] for c in ya], [c[todo] for c in fa], ha[todo], adaptive)
            ok = np.all(np.isfinite(np.stack(out)), axis=0) & np.isfinite(err)
            if not adaptive:
                st[todo[~ok]] = NONFINITE
                good = todo[ok]
                for c in range(6):
                    y1[c][good] = out[c][ok]
                taken[good] = ha[good]
                ta[good] = ta[good] + ha[good]
                break
            acc = ok & (err <= 1.1 * max_err)
            fac = np.where(ok, self.factor(max_err, np.where(ok, err, 1.0)), 0.2)
            good = todo[acc]
            for c in range(6):
                y1[c][good] = out[c][acc]
            taken[good] = ha[good]
            ta[good] = ta[good] + ha[good]
            ha[todo] = ha[todo] * fac
            rejections[todo[~acc]] += 1
            rej = todo[~acc]
            st[rej[rejections[rej] >= MAX_REJECTIONS]] = REJECTED
            todo = rej[rejections[rej] < MAX_REJECTIONS]
        run = st == RUNNING
        moved = run.copy()  # (a lane that stopped in its trials keeps its state; every other lane moves)
        ynew = [np.where(run, y1[c], ya[c]) for c in range(6)]
        f1, kin1 = self.rhs(ynew)
        bad = run & ~(np.all(np.isfinite(np.stack(f1)), axis=0) & np.isfinite(kin1))
        st[bad] = NONFINITE
        run = st == RUNNING
        eps1 = 0.5 * kin1 / (ynew[4] * ynew[4])
        ended = run & (eps1 >= 1.0)
        nend = n0 + (1.0 - eps0) / (eps1 - eps0) * (ynew[5] - n0)
        # the stop on N (inflx_bg_step_target): a lane that passes n_stop, unless the end of inflation came first
        hit = (run | ended) & (ynew[5] >= n_stop) & ~(ended & (nend < n_stop))
        st[ended & ~hit] = ENDED
        ne = n_end[idx]
        ne[ended & ~hit] = nend[ended & ~hit]
        tnew = ta.copy()
        if hit.any():
            w = np.flatnonzero(hit)
            th = _locate(ya[5][w], fa[5][w], ynew[5][w], f1[5][w], taken[w], n_stop)
            loc = [_hermite(ya[c][w], fa[c][w], ynew[c][w], f1[c][w], taken[w], th) for c in range(5)] + [np.full(w.size, n_stop)]
            tnew[w] = (ta[w] - taken[w]) + th * taken[w]
            o = self.eom(loc[0], loc[1], loc[2], loc[3], self.p)
            okl = np.all(np.isfinite(np.stack(loc)), axis=0) & np.isfinite(tnew[w]) & np.isfinite(0.5 * o[3] / (loc[4] * loc[4]))
            for c in range(6):
                ynew[c] = ynew[c].copy()
                ynew[c][w] = loc[c]
            fl, kl = self.rhs([c[w] for c in ynew])
            for c in range(6):
                f1[c] = np.array(f1[c])
                f1[c][w] = fl[c]
            kin1 = np.array(kin1)
            kin1[w] = kl
            st[w] = np.where(okl & np.all(np.isfinite(np.stack(fl)), axis=0) & np.isfinite(kl), TARGET, NONFINITE)
        kicked = (st == RUNNING) | (st == TARGET)
        if kicked.any():
            w = np.flatnonzero(kicked)
            dn = np.where(st[w] == TARGET, n_stop - n0[w], ynew[5][w] - n0[w])
            lanes = idx[w]
            if rng is None:
                xi0, xi1 = normals(seed, np.full(w.size, step, dtype=np.uint64), real[lanes], stream[lanes])
            else:
                xi = rng.standard_normal((w.size, 2))
                xi0, xi1 = xi[:, 0], xi[:, 1]
            yk = [c[w] for c in ynew]
            g = self.noise(yk[0], yk[1], self.p)
            H0 = yk[4]
            amp = noise_scale * (H0 / TWO_PI)
            diff, drift = amp * np.sqrt(dn), 0.5 * (amp * amp) * dn
            yk[0] = yk[0] + diff * (g[0] * xi0) - drift * g[3]
            yk[1] = yk[1] + diff * (g[1] * xi0 + g[2] * xi1) - drift * g[4]
            o = self.eom(yk[0], yk[1], yk[2], yk[3], self.p)
            f0 = self.rhs_from(yk, o)
            drho = (f0[4] - f1[4][w]) + 0.5 * (o[3] - kin1[w])
            radicand = H0 * H0 + drho / 3.0
            yk[4] = np.sqrt(radicand)
            fk = self.rhs_from(yk, o)
            fine = np.isfinite(radicand) & np.all(np.isfinite(np.stack(yk)), axis=0) & np.all(np.isfinite(np.stack(fk)), axis=0) & np.isfinite(o[3])
            epsk = 0.5 * o[3] / (yk[4] * yk[4])
            target = st[w] == TARGET
            st[w] = np.where(~fine, NONFINITE, np.where(target, TARGET, np.where(epsk >= 1.0, ENDED, RUNNING)))
            kick_end = fine & ~target & (epsk >= 1.0)
            ne[w[kick_end]] = yk[5][kick_end]
            by_kick[lanes[kick_end]] = True
            for c in range(6):
                ynew[c] = np.array(ynew[c])
                ynew[c][w] = yk[c]
                f1[c] = np.array(f1[c])
                f1[c][w] = fk[c]
            kin1 = np.array(kin1)
            kin1[w] = o[3]
        for c in range(6):
            y[c][idx] = np.where(moved, ynew[c], ya[c])
            f[c][idx] = np.where(moved, f1[c], fa[c])
        kin[idx] = np.where(moved, kin1, kina)
        t[idx], h[idx], status[idx], n_end[idx] = tnew, ha, st, ne


# ---- the moments, independently --------------------------------------------------------------------------------------------------------
def exact_moments(values):
    """(mean, m2, m3, m4) of a list of doubles in long double, the mean from ``math.fsum``"""
    v = [float(x) for x in values]
    mean = math.fsum(v) / len(v)
    d = np.array(v, dtype=np.longdouble) - np.longdouble(mean)
    return mean, *(float(np.sum(d**k) / len(v)) for k in (2, 3, 4))


# ---- the host build ----------------------------------------------------------------------------------------------------------------------
class StochasticTwin:
    """tests/stochastic_twin.cpp built for the CPU from an artefact's generated headers, contraction off like the other twins"""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        self.artifact = artifact
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.noise_header_text())
        sources = [os.path.join(CSRC, f) for f in ("inflx_background.h", "inflx_stochastic.h", "inflx_philox.h")] + [os.path.join(HERE, "stochastic_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_stochastic_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, noise_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".noise.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr, noise_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            subprocess.run([cxx, "-O2", "-fPIC", "-shared", "-o", tmp, *self.compile_options(hdr, eom_hdr, noise_hdr, contract), sources[-1]], check=True)
            os.replace(tmp, so)
        self.headers = (hdr, eom_hdr, noise_hdr)
        self.lib = lib = C.CDLL(so)
        lib.twin_philox.argtypes = [_UP, C.c_uint32, C.c_uint32, _UP]
        lib.twin_philox.restype = None
        lib.twin_uniform.argtypes = [C.c_uint32, C.c_uint32]
        lib.twin_uniform.restype = C.c_double
        lib.twin_normals.argtypes = [C.c_uint64, C.c_uint64, C.c_size_t, C.c_uint32, C.c_uint32, _DP]
        lib.twin_normals.restype = None
        lib.twin_noise_point.argtypes = [_DP, _DP, C.c_size_t, _DP]
        lib.twin_noise_point.restype = None
        lib.twin_stochastic.argtypes = [_DP, C.c_size_t, _DP, C.c_size_t, C.c_size_t, _UP, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_size_t, C.c_int, C.c_double,
                                        C.c_double, _DP, _DP]  # fmt: skip
        lib.twin_stochastic.restype = None
        lib.twin_moments.argtypes = [_DP, _DP, C.c_size_t, _DP]
        lib.twin_moments.restype = None

    @staticmethod
    def compile_options(hdr, eom_hdr, noise_hdr, contract="off"):
        """what any build of tests/stochastic_twin.cpp takes besides its output (the stand-alone program adds -DSTOCHASTIC_TWIN_MAIN)"""
        return ["-std=c++17", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_NOISE_HEADER="{noise_hdr}"']  # fmt: skip

    def philox(self, counter, key):
        c = (C.c_uint32 * 4)(*counter)
        out = (C.c_uint32 * 4)()
        self.lib.twin_philox(c, key[0], key[1], out)
        return list(out)

    def uniform(self, hi, lo):
        return self.lib.twin_uniform(hi, lo)

    def normals(self, seed, step_begin, n, r, stream):
        xi = np.empty((n, 2))
        self.lib.twin_normals(seed, step_begin, n, r, stream, xi.ctypes.data_as(_DP))
        return xi

    def noise_point(self, p, pts):
        p = np.ascontiguousarray(p, dtype=np.float64)
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        out = np.empty((pts.shape[0], 5))
        self.lib.twin_noise_point(p.ctypes.data_as(_DP), pts.ctypes.data_as(_DP), pts.shape[0], out.ctypes.data_as(_DP))
        return out

    def run(self, pars, init, R, *, streams=None, seed=0, noise_scale=1.0, dN_max=1.0 / 32.0, N_stop=None, max_steps=1_000_000, max_err=1e-8, solver="rkf",
            dt=None) -> StochasticResult:  # fmt: skip
        init = np.ascontiguousarray(init, dtype=np.float64).reshape(-1, 4)
        B = init.shape[0]
        p = np.ascontiguousarray(pars, dtype=np.float64)
        ids = np.ascontiguousarray(np.arange(B) if streams is None else streams, dtype=np.uint32)
        samples, accepted = np.empty((7, B * R)), np.empty(B * R)
        self.lib.twin_stochastic(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), B, R, ids.ctypes.data_as(_UP), seed, noise_scale,
                                 dN_max, math.nan if N_stop is None else N_stop, max_steps, 1 if solver == "rkf" else 0, max_err, dt or 0.0,
                                 samples.ctypes.data_as(_DP), accepted.ctypes.data_as(_DP))  # fmt: skip
        return StochasticResult(samples[0], samples[1:6].T.copy(), samples[6].astype(np.int64), accepted.astype(np.int64), None)

    def moments(self, N, status):
        """(12,): mean, m2, m3, m4, min, max, lanes per status, in the order of inflx_st_reduce"""
        N = np.ascontiguousarray(N, dtype=np.float64)
        st = np.ascontiguousarray(status, dtype=np.float64)
        out = np.empty(12)
        self.lib.twin_moments(N.ctypes.data_as(_DP), st.ctypes.data_as(_DP), N.size, out.ctypes.data_as(_DP))
        return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
SIGMA2 = 0.01  # (H / 2 pi)^2 of the two constant-potential cases
V_CONST = 3.0 * (2.0 * math.pi) ** 2 * SIGMA2
N_DIFFUSE = 8.0


@functools.lru_cache(maxsize=None)
def constant_model(curved: bool):
    """V = V0 on the flat plane, or on the hyperbolic plane G = diag(1, L^2 sinh^2(phi / L))"""
    from inflatox_amd import InflationModelBuilder

    phi, theta, v0, L = sp.symbols("phi theta V0 L")
    G = [[1, 0], [0, L**2 * sp.sinh(phi / L) ** 2]] if curved else [[1, 0], [0, 1]]
    name = "constant_hyperbolic" if curved else "constant_flat"
    # (a constant potential has no gradient direction: the builder's checks of the gradient basis are off, and nothing here uses it)
    return InflationModelBuilder.new([phi, theta], G, v0, model_name=name, init_sympy_printing=False, silent=True, simplify=False, assertions=False).build()


def named_pars(art, **values):
    p = np.zeros(art.n_parameters)
    for name, value in values.items():
        if name in art.symbol_dictionary:
            p[int(art.symbol_dictionary[name][5:-1])] = value
    return p


@functools.lru_cache(maxsize=None)
def constant_case(curved: bool, device: bool = False):
    """(artifact, p, init (1, 4), fixed dt with dN = 1/16) of an exact-diffusion case: chi = 0, so the state moves by its kicks alone"""
    from deltan_reference import host_artifact_of
    from inflatox_amd import Compiler

    model = constant_model(curved)
    art = Compiler(model, silent=True).compile() if device else host_artifact_of(model, name=model.model_name)
    p = named_pars(art, V0=V_CONST, L=1.0)
    H = math.sqrt(V_CONST / 3.0)
    return art, p, np.array([[1.5, 0.25, 0.0, 0.0]]), (1.0 / 16.0) / H


def diffusion_checks(curved, N, state, status, R):
    """Items 5 and 6 of the issue, shared with the GPU test: the z-scores, every one asserted within 5"""
    assert np.all(status == TARGET) and np.all(N == N_DIFFUSE)
    if not curved:
        var = SIGMA2 * N_DIFFUSE
        se = var * math.sqrt(2.0 / (R - 1))
        z = {"var0": (state[:, 0].var(ddof=1) - var) / se, "var1": (state[:, 1].var(ddof=1) - var) / se,
             "cov": np.cov(state[:, 0], state[:, 1])[0, 1] / (var / math.sqrt(R - 1))}  # fmt: skip
    else:
        want = math.cosh(1.5) * math.exp(SIGMA2 * N_DIFFUSE)
        c = np.cosh(state[:, 0])
        z = {"cosh": (c.mean() - want) / (c.std(ddof=1) / math.sqrt(R)), "martingale": (c.mean() - math.cosh(1.5) * math.exp(SIGMA2 * N_DIFFUSE / 2)) / (c.std(ddof=1) / math.sqrt(R))}
        print(f"hyperbolic plane: E[cosh phi] {c.mean():.6f}, exact {want:.6f}, without the Ito term {math.cosh(1.5) * math.exp(SIGMA2 * N_DIFFUSE / 2):.6f}")
    z = {k: float(v) for k, v in z.items()}
    print(f"exact diffusion ({'hyperbolic plane' if curved else 'flat chart'}), R = {R}: z-scores {z}")
    assert all(abs(v) <= 5.0 for k, v in z.items() if k != "martingale"), z
    return z


@functools.lru_cache(maxsize=None)
def hyperbolic_case():
    """(spec, artifact, model, p) of the hyperbolic example model"""
    import workloads

    spec, art = workloads.artifact_for("hyperbolic")
    return spec, art, workloads.model_for("hyperbolic"), np.asarray(spec.args, dtype=np.float64)


def restatement_of(model, artifact, p):
    return StochasticRestatement(model_functions(model, artifact.symbol_dictionary), noise_functions(model, artifact.symbol_dictionary), p)


# the lane-by-lane cases: (points (B, 4), fixed dt, steps) -- 600 steps cross two launch windows of 256
PARITY_POINTS = np.array([[7.3, 0.4, -0.8, 1e-4], [6.9, -0.7, -0.8, -2e-4], [7.6, 0.1, -0.8, 5e-5]])
# (noise_scale 0.2: at 1 the hyperbolic points are in the regime of eternal inflation, where some realisations run away and are chaotic)
PARITY_DT, PARITY_STEPS, PARITY_R, PARITY_SEED, PARITY_SCALE = 2e-2, 600, 130, 20240229, 0.2

# ... and EGNO on the GPU: three points of its sweep extent at rest, where V > 0 and H is about 1e-3.  EGNO's equations of motion cancel
# (tests/test_background.py), and its trajectories carry the rounding of an FMA on: at these points the host twin with and without
# contraction differs by 3e-10 after 600 steps of dt = 10 (6 e-folds) and by 2.4e-11 after 600 steps of dt = 1, so dt = 1 it is -- the
# kernels contract, the twin does not, and the bound has to see the kicks, not the model's conditioning.
EGNO_POINTS = np.array([[0.47, 1.2, 0.0, 0.0], [0.48, 2.0, 0.0, 0.0], [0.49, 0.8, 0.0, 0.0]])
EGNO_DT, EGNO_SCALE = 1.0, 1.0

# the comparison in law (independent random numbers): three hyperbolic points 8 to 12 e-folds before the end, adaptive rkf.
# noise_scale 0.4 gives std(N) / N of about 10 per cent there (recorded in profiles/background_stochastic.json)
LAW_POINTS = np.array([[7.3, 0.4, -0.8, 1e-4], [6.9, -0.7, -0.8, -2e-4], [7.6, 0.1, -0.8, 5e-5]])
LAW_SCALE, LAW_DN_MAX, LAW_R = 0.4, 0.125, 1 << 14


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound():
    """what a lane-by-lane difference may be: 1e-10 plus twice the twin's own difference with and without FMA contraction"""
    return 1e-10 + 2.0 * recorded()["d"]["worst"]


def lane_difference(a: StochasticResult, b: StochasticResult):
    """worst absolute difference of N and the five state components over the lanes (all of order 1 to 10); statuses must agree"""
    assert np.array_equal(a.status, b.status), (np.flatnonzero(a.status != b.status)[:10], a.status[:10], b.status[:10])
    return float(max(np.nanmax(np.abs(a.N - b.N)), np.nanmax(np.abs(a.state - b.state))))


def parity_cases():
    """(name, artifact, model, p, points) of the lane-by-lane cases on the host: hyperbolic and one model with G_01 != 0"""
    import background_truth as bt

    _spec, art, model, p = hyperbolic_case()
    yield "hyperbolic", art, model, p, PARITY_POINTS
    z = bt.zoo_model("skew")
    pts = np.array([[1.2, 0.3, -0.1, 0.05], [0.8, -0.5, 0.1, -0.05], [1.7, 1.0, -0.05, 0.02]])
    yield "skew", bt.host_artifact("skew"), z.model, np.array([1.0, 1.2, 0.8])[: bt.host_artifact("skew").n_parameters], pts


# ... and on a model with special functions (background_truth.special_model): I_0 in the metric reaches the kicks' Cholesky factor
# and I_1 the drift; three points of the box, per-point parameter rows, 200 steps like ``skew``
SPECIAL_MODEL = "bessel_skew"
SPECIAL_POINTS = np.array([[1.2, 0.3, -0.1, 0.05], [0.8, -0.5, 0.1, -0.05], [1.7, 1.0, -0.05, 0.02]])
SPECIAL_PARS = np.array([[1.0, 1.2, 2.4], [0.7, 1.6, 3.1], [1.5, 0.6, 2.0]])  # a, b, nu
SPECIAL_STEPS = 200


def special_run(run, solver):
    """``run(p, pts, R, **kw)`` -- a twin's ``run`` or the device's -- on the special-function case"""
    return run(SPECIAL_PARS, SPECIAL_POINTS, PARITY_R, seed=PARITY_SEED, noise_scale=PARITY_SCALE, max_steps=SPECIAL_STEPS, solver=solver, dt=PARITY_DT)


def measure_d_special():
    """``measure_d`` on the special-function case: {solver: worst difference}"""
    import background_truth as bt

    art = bt.host_artifact(SPECIAL_MODEL)
    d = {solver: lane_difference(*[special_run(StochasticTwin(art, contract=c).run, solver) for c in ("off", "fast")]) for solver in ("rk4", "rkf")}
    d["worst"] = max(d.values())
    return d


def bound_special():
    return 1e-10 + 2.0 * recorded()["d_" + SPECIAL_MODEL]["worst"]


def measure_d():
    """the twin with FMA contraction against the twin without, over the lane-by-lane cases: {case/solver: worst difference}"""
    d = {}
    for name, art, _model, p, pts in parity_cases():
        steps = PARITY_STEPS if name == "hyperbolic" else 200
        for solver in ("rk4", "rkf"):
            runs = [StochasticTwin(art, contract=c).run(p, pts, PARITY_R, seed=PARITY_SEED, noise_scale=PARITY_SCALE, max_steps=steps, solver=solver, dt=PARITY_DT)
                    for c in ("off", "fast")]  # fmt: skip
            d[f"{name}/{solver}"] = lane_difference(*runs)
            print(f"{name} {solver}: twin with FMA contraction against without, worst lane difference {d[f'{name}/{solver}']:.3e}", flush=True)
    d["worst"] = max(d.values())
    return d


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = recorded() if os.path.exists(PROFILE) else {}
    result["d"] = measure_d()
    result["d_" + SPECIAL_MODEL] = measure_d_special()
    result["d_what"] = ("worst absolute lane difference (N_end and the five state components) between the host twin built with -ffp-contract=fast -mfma and with "
                        "-ffp-contract=off, fixed dt, same Philox stream; tests assert 1e-10 + 2 x worst")  # fmt: skip
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
