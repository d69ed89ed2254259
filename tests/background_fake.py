"""A stand-in for the native layer under ``inflatox_amd.background``: a stub artefact that holds nothing but ``n_fields`` and
``n_parameters`` (and counts its ``ensure_*`` calls), and ``FakeLib``, whose methods have the signatures of the ``InflatoxDevLib``
background wrappers.  A method checks what it is handed the way the C ABI needs it (float64, C-contiguous, the documented shape),
records a copy of every argument, and returns arrays that depend on nothing but the position: ``value(lane, plane, sample)`` for
floating-point planes, ``N_END0 + lane`` for e-fold counts, and a status that cycles by lane through the method's entry of
``CYCLES``.  No device, no compiler."""

import types

import numpy as np

COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET, ENDED_SHORT, LOCATED = 0, 1, 2, 3, 4, 5, 6, 7
N_PARAMETERS = 3
#: the e-fold count every method returns for lane 0
N_END0 = 60.0
#: status by lane (lane modulo the length), per method; ``n_before``: the crossings' count of targets below ln H_0
CYCLES = {
    "solve_eom": (ENDED, ENDED, COMPLETE),
    "solve_eom_to_efolds": (TARGET, TARGET, ENDED),
    "solve_eom_sampled": (TARGET, ENDED, COMPLETE),
    "solve_eom_crossings": (TARGET, TARGET, COMPLETE),
    "n_before": (0, 1),
    "inflation_end": (ENDED, ENDED, COMPLETE),
    "transfer_functions": (ENDED, COMPLETE, TARGET),
    "mode_spectra": (ENDED, COMPLETE, TARGET),
    "mode_evolution": (ENDED, COMPLETE, TARGET),
    "delta_n": (LOCATED, COMPLETE + 16 * 4, LOCATED),
    "stochastic_efolds": (ENDED, ENDED, COMPLETE),
}
ENSURES = ("background", "kinematics", "masses", "transfer", "modes", "tensor", "deltan", "evolution", "stochastic", "distribution", "crossing")


def value(lane, plane=0, sample=0):
    """What the fake writes at (lane, plane, sample) of a floating-point result: positive, finite, different everywhere."""
    return 1.0 + lane + 100.0 * plane + 0.01 * sample


def stub_artifact(n_fields=2):
    """An artefact of ``n_fields`` fields and ``N_PARAMETERS`` parameters whose ``ensure_<what>()`` append ``<what>`` to ``ensured``"""
    art = types.SimpleNamespace(n_fields=n_fields, n_parameters=N_PARAMETERS, ensured=[])
    for what in ENSURES:
        setattr(art, "ensure_" + what, lambda what=what: art.ensured.append(what))
    return art


def _planes(shape, lane, plane=None, sample=None):
    idx = np.indices(shape)
    return value(idx[lane], 0 if plane is None else idx[plane], 0 if sample is None else idx[sample])


def _f64(a, shape, what):
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous, (what, type(a), getattr(a, "dtype", None))
    assert a.shape == shape, (what, a.shape, shape)


class FakeLib:
    device = 0

    def __init__(self, cycles=None):
        self.calls = []  # (method, {argument: copy})
        self.cycles = {**CYCLES, **(cycles or {})}

    def _record(self, name, **args):
        self.calls.append((name, {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in args.items()}))

    def _cycle(self, name, n, dtype=np.int8):
        cycle = self.cycles[name]
        return np.array([cycle[i % len(cycle)] for i in range(n)], dtype=dtype)

    def _rows(self, p, n):
        """parameter rows: (n_par,) shared, or one row per lane"""
        assert isinstance(p, np.ndarray) and p.dtype == np.float64 and p.flags.c_contiguous, ("p", type(p))
        assert p.shape in ((N_PARAMETERS,), (n, N_PARAMETERS)), ("p", p.shape, n)

    def _init(self, p, init):
        assert init.ndim == 2, init.shape
        B = init.shape[0]
        _f64(init, (B, 4), "init")
        self._rows(p, B)
        return B

    def _samples(self, samples):
        _f64(samples, (samples.size,), "samples")
        return samples.size

    @staticmethod
    def _scalars(ints=(), floats=()):
        assert all(type(v) is int for v in ints), ints
        assert all(type(v) is float for v in floats), floats

    def named(self, name):
        return [args for method, args in self.calls if method == name]

    # ---- the wrappers ----------------------------------------------------------------------------------------------------------------
    def solve_eom(self, p, init, rows, substeps, method, max_err, dt, flags):
        B = self._init(p, init)
        self._scalars((rows, substeps, method, flags), (max_err, dt))
        self._record("solve_eom", p=p, init=init, rows=rows, substeps=substeps, method=method, max_err=max_err, dt=dt, flags=flags)
        final_only = bool(flags & 2)
        states = _planes((B, 6), 0, 1) if final_only else _planes((B, rows, 6), 0, 2, 1)
        t = _planes((B,), 0) + 6000.0 if final_only else _planes((B, rows), 0, None, 1) + 6000.0
        return states, t, N_END0 + np.arange(B), self._cycle("solve_eom", B), np.arange(B, dtype=np.int64) % rows

    def solve_eom_to_efolds(self, p, init, target, max_steps, method, max_err, dt, flags):
        B = self._init(p, init)
        _f64(target, (B,), "target")
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("solve_eom_to_efolds", p=p, init=init, target=target, max_steps=max_steps, method=method, max_err=max_err, dt=dt, flags=flags)
        return _planes((B, 6), 0, 1), value(np.arange(B), 6), value(np.arange(B), 7), N_END0 + np.arange(B), self._cycle("solve_eom_to_efolds", B)

    def solve_eom_sampled(self, p, init, samples, max_steps, method, max_err, dt, flags):
        B, S = self._init(p, init), self._samples(samples)
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("solve_eom_sampled", p=p, init=init, samples=samples, max_steps=max_steps, method=method, max_err=max_err, dt=dt, flags=flags)
        return _planes((S, 8, B), 2, 1, 0), N_END0 + np.arange(B), self._cycle("solve_eom_sampled", B), np.full(B, S, dtype=np.uint32)

    def solve_eom_crossings(self, p, init, offset, samples, max_steps, method, max_err, dt, flags):
        B, S = self._init(p, init), self._samples(samples)
        _f64(offset, (B,), "offset")
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("solve_eom_crossings", p=p, init=init, offset=offset, samples=samples, max_steps=max_steps, method=method, max_err=max_err, dt=dt, flags=flags)
        return (_planes((S, 8, B), 2, 1, 0), N_END0 + np.arange(B), self._cycle("solve_eom_crossings", B), np.full(B, S, dtype=np.uint32),
                self._cycle("n_before", B, np.uint32))  # fmt: skip

    def inflation_end(self, p, init, max_steps, method, max_err, dt):
        B = self._init(p, init)
        self._scalars((max_steps, method), (max_err, dt))
        self._record("inflation_end", p=p, init=init, max_steps=max_steps, method=method, max_err=max_err, dt=dt)
        return _planes((B, 6), 0, 1), value(np.arange(B), 6), value(np.arange(B), 7), self._cycle("inflation_end", B)

    def _state_pass(self, name, planes, p, states, n, ld, traj_len):
        assert isinstance(states, np.ndarray) and states.dtype == np.float64 and states.strides[-1] == 8, name
        assert n % traj_len == 0 and ld >= 5
        self._rows(p, n // traj_len)
        self._record(name, p=p, states=states, n=n, ld=ld, traj_len=traj_len)
        return _planes((planes, n), 1, 0)

    def kinematics(self, p, states, n, ld, traj_len=1):
        return self._state_pass("kinematics", 6, p, states, n, ld, traj_len)

    def masses(self, p, states, n, ld, traj_len=1):
        return self._state_pass("masses", 8, p, states, n, ld, traj_len)

    def transfer_functions(self, p, init, dq_dn, samples, max_steps, method, max_err, dt, flags):
        B, S = self._init(p, init), self._samples(samples)
        if dq_dn is not None:
            _f64(dq_dn, (B,), "dq_dn")
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("transfer_functions", p=p, init=init, dq_dn=dq_dn, samples=samples, max_steps=max_steps, method=method, max_err=max_err, dt=dt, flags=flags)
        return _planes((S, 10, B), 2, 1, 0), _planes((B, 2), 0, 1), N_END0 + np.arange(B), self._cycle("transfer_functions", B), np.full(B, S, dtype=np.uint32)

    def mode_spectra(self, p, init, kappa, n_target, max_steps, method, max_err, dt, flags):
        n = self._init(p, init)
        _f64(kappa, (n,), "kappa")
        _f64(n_target, (n,), "n_target")
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("mode_spectra", p=p, init=init, kappa=kappa, n_target=n_target, max_steps=max_steps, method=method, max_err=max_err, dt=dt, flags=flags)
        return _planes((8 if flags & 8 else 22, n), 1, 0), N_END0 + np.arange(n), self._cycle("mode_spectra", n)

    def mode_evolution(self, p, init, kappa, n_target, shift, samples, max_steps, method, max_err, dt, flags):
        n, S = self._init(p, init), self._samples(samples)
        for name, a in (("kappa", kappa), ("n_target", n_target), ("shift", shift)):
            _f64(a, (n,), name)
        self._scalars((max_steps, method, flags), (max_err, dt))
        self._record("mode_evolution", p=p, init=init, kappa=kappa, n_target=n_target, shift=shift, samples=samples, max_steps=max_steps, method=method,
                     max_err=max_err, dt=dt, flags=flags)  # fmt: skip
        return _planes((22, n), 1, 0), _planes((S, 6, n), 2, 1, 0), N_END0 + np.arange(n), self._cycle("mode_evolution", n)

    def delta_n(self, p, centre, vel, rule, h0, h1, h_end, max_steps, method, max_err, dt):
        B = self._init(p, centre)
        if vel is not None:
            _f64(vel, (B, 9, 2), "vel")
        if h_end is not None:
            _f64(h_end, (B,), "h_end")
        self._scalars((rule, max_steps, method), (h0, h1, max_err, dt))
        self._record("delta_n", p=p, centre=centre, vel=vel, rule=rule, h0=h0, h1=h1, h_end=h_end, max_steps=max_steps, method=method, max_err=max_err, dt=dt)
        return _planes((21, B), 1, 0), _planes((2, B), 1, 0), self._cycle("delta_n", B, np.int32)

    def _streams(self, streams, B):
        if streams is not None:
            assert isinstance(streams, np.ndarray) and streams.dtype == np.uint32 and streams.flags.c_contiguous and streams.shape == (B,), "streams"

    def stochastic_efolds(self, p, init, R, streams, seed, noise_scale, dn_max, n_stop, max_steps, method, max_err, dt, want_samples=False):
        B = self._init(p, init)
        self._streams(streams, B)
        self._scalars((R, seed, max_steps, method), (noise_scale, dn_max, n_stop, max_err, dt))
        self._record("stochastic_efolds", p=p, init=init, R=R, streams=streams, seed=seed, noise_scale=noise_scale, dn_max=dn_max, n_stop=n_stop, max_steps=max_steps,
                     method=method, max_err=max_err, dt=dt, want_samples=want_samples)  # fmt: skip
        moments = _planes((12, B), 1, 0)
        moments[6:] = float(R) * (self._cycle("stochastic_efolds", B)[None, :] == np.arange(6)[:, None])  # every realisation of a point stops alike
        samples = None
        if want_samples:
            samples = _planes((7, B * R), 1, 0)
            samples[6] = np.repeat(self._cycle("stochastic_efolds", B), R)
        return moments, samples

    def stochastic_distribution(self, p, init, R, streams, seed, first, lanes_per_point, noise_scale, dn_max, max_steps, method, max_err, dt, bins, ranges):
        B = self._init(p, init)
        self._streams(streams, B)
        assert ranges.shape in ((1, 2), (B, 2))
        _f64(ranges, ranges.shape, "ranges")
        self._scalars((R, seed, first, lanes_per_point, max_steps, method, bins), (noise_scale, dn_max, max_err, dt))
        self._record("stochastic_distribution", p=p, init=init, R=R, streams=streams, seed=seed, first=first, lanes_per_point=lanes_per_point, noise_scale=noise_scale,
                     dn_max=dn_max, max_steps=max_steps, method=method, max_err=max_err, dt=dt, bins=bins, ranges=ranges)  # fmt: skip
        idx = np.indices((B, bins + 2))
        hist = (idx[0] + 1000 * idx[1]).astype(np.uint32)
        idx = np.indices((B, 6))
        return hist, (idx[0] + 1000 * idx[1]).astype(np.uint32)
