"""Background trajectories: the model's equations of motion integrated on the GPU.

``solve_eom`` is the reference's ``inflatox.background.solve_eom`` (python/inflatox/background.py) -- same signature, defaults and
return value.  ``solve_eom_batch`` integrates many initial conditions or parameter rows at once, one GPU lane per trajectory, and
``efolds_map`` places initial conditions on a sweep grid and returns the number of e-folds at the end of inflation there: the
counterpart of a consistency map from ``GeneralisedAL.complete_analysis`` over the same grid.  ``state_at_efolds`` returns the
state at which a trajectory has made a given number of e-folds, and ``horizon_exit_map`` the state N_star e-folds before the end
of inflation from every grid point: the (phi, chi, H) at which ``complete_analysis_ot`` and ``calc_V_array`` are evaluated.
``solve_eom_sampled`` returns every trajectory's state at one list of e-fold counts (or times) shared by all of them.
``solve_eom_batch_device`` is ``solve_eom_batch`` with the trajectories left on the GPU as ``torch`` tensors.
``kinematics`` evaluates epsilon_H, eta_parallel, the turn rate per e-fold and the gradient along and across the velocity at any of
these states -- host arrays, or the device-resident rows of ``solve_eom_batch_device`` without a byte crossing PCIe -- and
``turn_rate_map`` is ``horizon_exit_map`` followed by ``kinematics``: the measured counterpart, over the same grid, of what
``GeneralisedAL.complete_analysis`` predicts from the potential alone.  ``masses`` evaluates the second-order counterpart at the same
states -- the covariant Hesse matrix on the trajectory's own tangent and normal, the Ricci scalar of field space and the two entropic
masses built from them -- and ``mass_map`` is ``horizon_exit_map`` followed by it.  ``transfer_functions`` integrates the two
super-horizon perturbation equations whose coefficients are that turn rate and that mass along every trajectory -- T_RS, the
curvature perturbation sourced after horizon exit, and T_SS, the isocurvature that survives -- and ``transfer_map`` is
``horizon_exit_map`` followed by it, from every exit state to the end of inflation.  ``power_spectra`` integrates the full linear
mode equations from the Bunch-Davies vacuum inside the horizon, one GPU lane per (trajectory, wavenumber) -- the curvature and
isocurvature power spectra P_R and P_S and their correlation C_RS, with everything that sets the amplitude and the correlation at
horizon exit -- and ``spectrum_map`` is ``horizon_exit_map`` followed by it.  ``tensor_spectra`` is its tensor twin, the tensor power
spectrum P_T from one complex tensor amplitude per lane; ``observables`` differences both in ln k around a pivot of the trajectory's
own -- the scalar tilt n_s, its running, the tensor tilt n_t and the tensor-to-scalar ratio r -- and ``observables_map`` is
``horizon_exit_map`` followed by it: n_s and r, as maps, of the mode that leaves the horizon N_star e-folds before the end of inflation.
``delta_N`` runs nine-trajectory stencils around given states to one surface of uniform density each and differences the e-fold counts
-- N_,I, N_,IJ, the covariant second derivative and the local non-Gaussianity f_NL of the delta-N expansion -- and ``fnl_map`` is
``horizon_exit_map`` followed by it.  ``spectra_evolution`` is ``power_spectra`` with every mode's spectra sampled at a list of e-fold counts
along its evolution, from one integration of every lane; ``evolution_map`` is ``horizon_exit_map`` followed by it, and
``transfer_from_spectra`` reads the transfer functions T_RS and T_SS off such samples: the measured counterpart of ``transfer_functions``.
``stochastic_efolds`` adds the Langevin noise of the separate-universe picture to every trajectory -- a field kick of variance (H / 2 pi)^2
per e-fold, right on a curved field space -- and returns the moments of the e-fold count over many realisations of every point, the
input of the stochastic delta-N formalism; ``stochastic_map`` places the points on a sweep grid.  ``stochastic_distribution`` returns the
distribution P(N) itself, a histogram per point over up to 2^32 - 1 realisations run on GPU lanes that are used again as realisations
finish, and ``stochastic_distribution_map`` places the points on a sweep grid; ``distribution_pdf``, ``distribution_survival``,
``distribution_mean`` and ``distribution_tail_rate`` read a density, the survival function, the mean and the rate of an exponential
tail off such a histogram on the host.  ``horizon_crossings`` returns every trajectory's state where the comoving Hubble scale
ln(a H) reaches the points of one list of wavenumbers shared by all of them, located inside the accepted step like ``state_at_efolds``
locates N, and ``inflation_end`` the state where epsilon_H = 1 on the same dense output.  On top of them ``power_spectra_at_k``,
``tensor_spectra_at_k`` and ``observables_at_k`` are ``power_spectra``, ``tensor_spectra`` and ``observables`` on a k-grid common to all
trajectories; ``reheating_offset`` turns a physical wavenumber today and a reheating history into the offset of that grid, and
``pivot_exit_map`` and ``pivot_observables_map`` draw the exit state, N_star, n_s and r of such a pivot scale over a sweep grid, N_star
following from every trajectory instead of being guessed.  ``set_sf_errors`` chooses, for a model with special functions, between an
error and NaN where a function's domain is left.

The system (Planck units, cosmic time) is the reference's, y = (phi^0, phi^1, chi^0, chi^1, H) plus the e-fold count N::

    dphi^a/dt = chi^a,   dchi^a/dt = -eom^a(phi, chi) - 3 H chi^a,   dH/dt = V - 3 H^2,   dN/dt = H

with eom^a = Gamma^a_bc chi^b chi^c + G^ab d_b V the model's ``eom_fields``.  H starts from the Friedmann constraint
H0 = sqrt((V + G_ab chi^a chi^b / 2) / 3); epsilon_H = (G_ab chi^a chi^b / 2) / H^2.  The steppers and the step-size control are
described in csrc/inflx_background.h and DESIGN.md ("Background trajectories"); the kernels are csrc/inflx_background_kernels.hip,
built into ``<artefact>.background`` on first use (``CompilationArtifact.ensure_background``).
"""

from __future__ import annotations

import contextlib
import math
import operator
from typing import NamedTuple

import numpy as np

from . import _native
from ._native import InflatoxShapeError
from .compiler import CompilationArtifact

__all__ = ["solve_eom", "solve_eom_batch", "solve_eom_batch_device", "efolds_map", "state_at_efolds", "horizon_exit_map", "solve_eom_sampled", "EoMSolution", "EfoldsState",
           "SampledSolution", "STATUS", "kinematics", "turn_rate_map", "Kinematics", "masses", "mass_map", "Masses", "transfer_functions", "transfer_map",
           "TransferSolution", "power_spectra", "spectrum_map", "PowerSpectra", "tensor_spectra", "TensorSpectra", "observables", "Observables", "observables_map",
           "delta_N", "DeltaN", "fnl_map", "delta_N_status", "spectra_evolution", "SpectraEvolution", "evolution_map", "transfer_from_spectra",
           "stochastic_efolds", "stochastic_map", "StochasticEfolds", "stochastic_distribution", "stochastic_distribution_map", "StochasticDistribution",
           "distribution_pdf", "distribution_survival", "distribution_mean", "distribution_tail_rate", "horizon_crossings", "CrossingSolution", "inflation_end",
           "InflationEnd", "power_spectra_at_k", "tensor_spectra_at_k", "ExitPoints", "observables_at_k", "reheating_offset", "pivot_exit_map",
           "pivot_observables_map", "OUTSIDE_AT_START", "set_sf_errors"]  # fmt: skip

#: ``status`` codes of a trajectory (include/inflx_hip.h ``inflx_eom_status``)
COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5
#: ``horizon_exit_map`` only (no kernel status): inflation ended, but after fewer than N_star e-folds
ENDED_SHORT = 6
#: ``delta_N`` only (csrc/inflx_deltan.h): the trajectory met its surface / started at or past it
LOCATED, PAST_SURFACE = 7, 8
STATUS = {
    COMPLETE: "every requested step was taken",
    ENDED: "epsilon_H reached 1 (stop_at_end)",
    NONFINITE: "the state or the equations of motion at it are not finite",
    REJECTED: "50 consecutive rejected steps",
    UNDERFLOW: "the step size no longer moves t",
    TARGET: "N reached its target (state_at_efolds, horizon_exit_map); every sample was emitted (solve_eom_sampled)",
    ENDED_SHORT: "epsilon_H reached 1 after fewer than N_star e-folds (horizon_exit_map)",
    LOCATED: "the trajectory met its surface of uniform density (delta_N)",
    PAST_SURFACE: "the initial H is already at or below the surface's (delta_N)",
}
_METHODS = {"rk4": _native.EOM_RK4, "rkf": _native.EOM_RKF}


class EoMSolution(NamedTuple):
    """What :func:`solve_eom_batch` returns.  ``states`` (B, steps, 5): phi^0, phi^1, chi^0, chi^1, H (a strided view); ``t`` and
    ``N`` (B, steps): cosmic time and e-folds of every row; ``status`` (B,) int8: ``STATUS`` codes; ``last_row`` (B,): the last row
    that holds a state -- the rows after it are NaN; ``N_end`` (B,): N at epsilon_H = 1 with ``stop_at_end``, NaN otherwise.
    From :func:`solve_eom_batch_device`, ``states``, ``t`` and ``N`` are torch tensors on the GPU instead."""

    states: np.ndarray
    t: np.ndarray
    N: np.ndarray
    status: np.ndarray
    last_row: np.ndarray
    N_end: np.ndarray


class EfoldsState(NamedTuple):
    """What :func:`state_at_efolds` returns.  ``state`` (B, 5): phi^0, phi^1, chi^0, chi^1, H where N = ``N_target``; ``t``, ``N``
    and ``eps_H`` (B,): cosmic time, e-folds (the target) and epsilon_H there -- all NaN unless ``status`` (B,) int8 is ``TARGET``;
    ``N_end`` (B,): N at epsilon_H = 1 of a trajectory that ENDED before its target (``stop_at_end``), NaN otherwise."""

    state: np.ndarray
    t: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


class SampledSolution(NamedTuple):
    """What :func:`solve_eom_sampled` returns.  ``states`` (B, S, 5): phi^0, phi^1, chi^0, chi^1, H at every sample; ``t``, ``N`` and
    ``eps_H`` (B, S): cosmic time, e-folds and epsilon_H there -- all four are views of one (S, 8, B) array, trajectory fastest, and
    NaN for a sample the trajectory did not reach; ``n_stored`` (B,): the samples emitted, always the first ``n_stored``; ``N_end``
    (B,): N at epsilon_H = 1 of a trajectory that ENDED (``stop_at_end``), NaN otherwise; ``status`` (B,) int8: ``TARGET`` when all
    S samples were emitted."""

    states: np.ndarray
    t: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    n_stored: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


def _dylib(artifact: CompilationArtifact, background: bool = True) -> _native.InflatoxDevLib:
    """The artefact's background object (built on first use; ``kinematics`` does without it) and one handle per artefact, opened on
    device 0 without the basis check."""
    if background:
        artifact.ensure_background()
    lib = getattr(artifact, "_background_dylib", None)
    if lib is None:
        lib = _native.InflatoxDevLib(artifact.shared_object_path)
        artifact._background_dylib = lib
    return lib


def set_sf_errors(artifact: CompilationArtifact, mode: str) -> None:
    """What the functions of this module do when a ``Compiler(link_gsl=True)`` model evaluated a Bessel or hypergeometric function
    outside its domain -- the words and errors of ``GeneralisedAL(..., sf_errors=)``, applied to the artefact's background handle
    (opened here when no call has opened it yet) and kept for every later call on the artefact.  ``"raise"`` (the default of such an
    artefact): ``kinematics`` and ``masses`` raise :class:`InflatoxSpecialFunctionError` when a state lies outside the domain, and a
    call that integrates trajectories raises it when one of them stopped ``NONFINITE`` there; a trial step that left the domain and was
    retried with a shorter one raises nothing.  An ADAPTIVE trajectory that really reaches a domain's edge does not become ``NONFINITE``:
    every trial that crosses the edge is retried shorter, the steps pile up in front of it and the trajectory stops ``UNDERFLOW`` --
    it signals the exit through that status, not through the error; a fixed ``dt`` or a start outside the domain gives ``NONFINITE``.
    ``"nan"``: every call returns its result, with NaN and ``NONFINITE`` where the domain
    was left -- an ``efolds_map`` whose grid touches a domain edge holds NaN at those points."""
    _native._sf_policy(mode)  # (a wrong word is refused before the handle is opened)
    _dylib(artifact, background=False).set_sf_errors(mode)


def _check_common(artifact, steps, max_err, solver, dt, substeps=1):
    if getattr(artifact, "n_fields", None) != 2:
        raise InflatoxShapeError(f"the background solver requires a 2-field model (model has {getattr(artifact, 'n_fields', None)} fields)")
    try:
        steps = operator.index(steps)
        substeps = operator.index(substeps)
    except TypeError:
        raise ValueError("steps and substeps must be integers") from None
    if steps < 1:
        raise ValueError(f"steps must be at least 1 (got {steps})")
    if substeps < 1 or substeps >= 2**32:
        raise ValueError(f"substeps must be in [1, 2^32) (got {substeps})")
    if (steps - 1) * substeps > 2**62:
        raise ValueError("steps x substeps exceeds 2^62 accepted steps")
    max_err = float(max_err)
    if not (max_err > 0.0 and math.isfinite(max_err)):
        raise ValueError(f"max_err must be a positive finite number (got {max_err})")
    if solver not in _METHODS:
        raise ValueError(f"unknown solver {solver!r}: choose 'rk4' or 'rkf'")
    if dt is not None:
        dt = float(dt)
        if not (dt > 0.0 and math.isfinite(dt)):
            raise ValueError(f"dt must be None (adaptive) or a positive finite step (got {dt})")
    return steps, substeps, max_err, dt


def _pars(artifact, pars, B):
    p = np.ascontiguousarray(pars, dtype=np.float64)
    n = artifact.n_parameters
    if p.ndim <= 1:
        if p.size != n:
            raise InflatoxShapeError(f"model has {n} parameters (got {p.size})")
        return p.reshape(n)
    if p.ndim != 2 or p.shape != (B, n):
        raise InflatoxShapeError(f"pars must have shape ({n},) or ({B}, {n}) (got {p.shape})")
    return p


def _check_fields(fields_init, derivatives_init):
    x = np.ascontiguousarray(fields_init, dtype=np.float64)
    v = np.ascontiguousarray(derivatives_init, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 2 or v.shape != x.shape:
        raise InflatoxShapeError(f"fields_init and derivatives_init must both have shape (B, 2) (got {x.shape} and {v.shape})")
    return x, v


def _check_samples(samples, name, noun, negative=False):
    """A list of points shared by all trajectories, the argument ``name`` holding ``noun``: (S,) float64 with 1 <= S < 2^32, finite,
    strictly increasing and, unless ``negative``, >= 0."""
    try:
        pts = np.ascontiguousarray(samples, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be convertible to a float64 array") from None
    if pts.ndim != 1:
        raise InflatoxShapeError(f"{name} must be one-dimensional (got shape {pts.shape})")
    if pts.size < 1 or pts.size >= 2**32:
        raise ValueError(f"the number of {noun} must be in [1, 2^32) (got {pts.size})")
    if negative:
        if not np.isfinite(pts).all():
            raise ValueError(f"{name} must be finite")
    elif not (np.isfinite(pts).all() and (pts >= 0.0).all()):
        raise ValueError(f"{name} must be finite and >= 0")
    if not (np.diff(pts) > 0.0).all():
        raise ValueError(f"{name} must be strictly increasing")
    return pts


def _check_n_star(N_star):
    try:
        N_star = float(N_star)
    except (TypeError, ValueError):
        raise ValueError("N_star must be a number") from None
    if not (math.isfinite(N_star) and N_star >= 0.0):
        raise ValueError(f"N_star must be finite and >= 0 (got {N_star})")
    return N_star


def _check_grid(start_stop, N0, N1, derivatives_init):
    """The grid of a map and the velocities its trajectories start with: (start_stop as an array of four, N0, N1, d (2,))."""
    ss = np.asarray(start_stop, dtype=np.float64)
    if ss.size != 4:
        raise InflatoxShapeError(f"start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape {ss.shape})")
    N0, N1 = operator.index(N0), operator.index(N1)
    if N0 < 1 or N1 < 1:
        raise ValueError(f"the grid needs at least one point per axis (got {N0} x {N1})")
    d = np.asarray(derivatives_init, dtype=np.float64).reshape(-1)
    if d.size != 2:
        raise InflatoxShapeError(f"derivatives_init must hold two velocities (got {d.size})")
    return ss, N0, N1, d


def _parameter_row(artifact, pars, who):
    """The one parameter row of a map; ``who``: the map and its verb, for the message."""
    p = _pars(artifact, pars, 1)
    if p.ndim != 1:
        raise InflatoxShapeError(f"{who} one parameter row")
    return p


def _grid_init(start_stop, N0, N1, d):
    """The initial conditions (N0 N1, 4) of a map's trajectories, point i N1 + j at (x0[i], x1[j]) of ``grid_points`` with the
    velocities ``d``."""
    x0, x1 = grid_points(start_stop, N0, N1)
    init = np.empty((N0 * N1, 4))
    init[:, 0] = np.repeat(x0, N1)
    init[:, 1] = np.tile(x1, N0)
    init[:, 2:] = d
    return init


def _second_stage(state, status, status_dtype, planes, feature, run=None):
    """The second stage of a two-stage map.  ``state`` (..., 5) and ``status`` (...) are the first stage's; ``run`` are the flat
    indices of the lanes that go on (None: those whose status is ``TARGET``).  ``feature(x, v, run)`` runs on their fields and
    velocities and returns one array per plane, (n, *planes[i]), and the lanes' status.  Returns (the planes, (..., *planes[i]) each
    and NaN on every other lane; ``status`` as ``status_dtype``, overwritten on the lanes that ran)."""
    lead = status.shape
    flat = state.reshape(-1, 5)
    status = status.astype(status_dtype).reshape(-1)
    out = [np.full((status.size, *shape), np.nan) for shape in planes]
    if run is None:
        run = np.flatnonzero(status == TARGET)
    if run.size:
        values, status[run] = feature(flat[run, :2], flat[run, 2:4], run)
        for plane, got in zip(out, values):
            plane[run] = got
    return [plane.reshape(*lead, *shape) for plane, shape in zip(out, planes)], status.reshape(lead)


def _companion_dylib(artifact, *what):
    """The artefact's handle, with the companion objects ``what`` built first (``CompilationArtifact.ensure_<what>``)."""
    for name in what:
        getattr(artifact, "ensure_" + name)()
    return _dylib(artifact, background=False)


@contextlib.contextmanager
def _side_stream(artifact, device, *tensors):
    """The artefact's own torch stream, as an integer, for a native call on ``tensors``: ordered after what torch's current stream of
    ``device`` has enqueued (the tensors were written or allocated there); afterwards the current stream is ordered after the call and
    the tensors are recorded on the side stream."""
    import torch

    if getattr(artifact, "_background_torch_stream", None) is None:
        artifact._background_torch_stream = torch.cuda.Stream(device=device)
    side = artifact._background_torch_stream
    consumer = torch.cuda.current_stream(device)
    side.wait_stream(consumer)
    yield side.cuda_stream
    consumer.wait_stream(side)
    for tensor in tensors:
        tensor.record_stream(side)


def _check_batch(artifact, pars, steps, fields_init, derivatives_init, max_err, solver, dt, substeps):
    """The argument checks of ``solve_eom_batch`` and ``solve_eom_batch_device``: (steps, substeps, max_err, dt, p, init (B, 4))."""
    steps, substeps, max_err, dt = _check_common(artifact, steps, max_err, solver, dt, substeps)
    x, v = _check_fields(fields_init, derivatives_init)
    p = _pars(artifact, pars, x.shape[0])
    return steps, substeps, max_err, dt, p, np.concatenate([x, v], axis=1)


def solve_eom_batch(artifact: CompilationArtifact, pars, steps: int, fields_init, derivatives_init, max_err: float = 1e-6, solver: str = "rkf", *,
                    dt: float | None = None, substeps: int = 1, stop_at_end: bool = False) -> EoMSolution:  # fmt: skip
    """B trajectories at once, one GPU lane each.  ``fields_init`` and ``derivatives_init`` are (B, 2); ``pars`` is (n_par,),
    shared by every trajectory, or (B, n_par).  Row 0 of a trajectory is its initial state, row k the state after k*``substeps``
    accepted steps.  ``solver``: ``"rkf"`` (Fehlberg 4(5)) or ``"rk4"`` (classical RK4, error from step doubling); ``max_err``: the
    bound of the adaptive step on the absolute Euclidean norm of the error over phi, chi and H; ``dt``: a fixed step without error
    control instead.  ``stop_at_end``: a trajectory stops at the first accepted step where epsilon_H >= 1 -- the row that step falls in
    holds the state there, ``N_end`` the e-fold count at epsilon_H = 1, linear in epsilon_H across the step (see ``efolds_map`` for
    its accuracy); a trajectory that starts with epsilon_H >= 1 ends at once, with ``N_end`` = 0 and row 0 its last row.  A trajectory
    that stops for another reason (``status``) has NaN rows from there on.  However large ``substeps``, no kernel launch takes more
    than 256 accepted steps per trajectory (a row may span launches).  Bad arguments raise before anything runs on the device."""
    steps, substeps, max_err, dt, p, init = _check_batch(artifact, pars, steps, fields_init, derivatives_init, max_err, solver, dt, substeps)
    flags = _native.EOM_STOP_AT_END if stop_at_end else 0
    states, t, n_end, status, last_row = _dylib(artifact).solve_eom(p, init, steps, substeps, _METHODS[solver], max_err, dt or 0.0, flags)
    return EoMSolution(states[:, :, :5], t, states[:, :, 5], status, last_row, n_end)


def solve_eom_batch_device(artifact: CompilationArtifact, pars, steps: int, fields_init, derivatives_init, max_err: float = 1e-6, solver: str = "rkf", *,
                           dt: float | None = None, substeps: int = 1, stop_at_end: bool = False) -> EoMSolution:  # fmt: skip
    """``solve_eom_batch`` with a DEVICE-RESIDENT result: the same arguments, checked in the same order before torch or the device is
    touched, and the same values bit for bit.  ``states`` (B, steps, 5), ``t`` and ``N`` (B, steps) are ``torch.float64`` tensors on
    the GPU of the artefact's handle -- views of one (B, steps, 6) and one (B, steps) tensor, written there by the transpose kernel:
    no row crosses PCIe.  They speak DLPack (``__dlpack__``) and ``__cuda_array_interface__``, so CuPy / JAX / numba consumers take
    them without a copy.  ``status``, ``last_row`` and ``N_end`` are numpy arrays as in ``solve_eom_batch``.  As for
    ``GeneralisedAL.complete_analysis_device``, the run is ordered after what torch's current stream has enqueued and torch's current
    stream is ordered after the run: the tensors can be used like the result of any torch operation."""
    steps, substeps, max_err, dt, p, init = _check_batch(artifact, pars, steps, fields_init, derivatives_init, max_err, solver, dt, substeps)
    flags = _native.EOM_STOP_AT_END if stop_at_end else 0
    import torch

    lib = _dylib(artifact)
    B = init.shape[0]
    device = torch.device("cuda", lib.device)
    states = torch.empty((B, steps, 6), dtype=torch.float64, device=device)
    t = torch.empty((B, steps), dtype=torch.float64, device=device)
    if B:
        with _side_stream(artifact, device, states, t) as stream:
            n_end, status, last_row = lib.solve_eom_device(p, init, steps, substeps, _METHODS[solver], max_err, dt or 0.0, flags, states.data_ptr(),
                                                           states.numel() * 8, t.data_ptr(), t.numel() * 8, stream=stream)  # fmt: skip
    else:
        n_end, status, last_row = np.empty(0), np.empty(0, dtype=np.int8), np.empty(0, dtype=np.int64)
    return EoMSolution(states[:, :, :5], t, states[:, :, 5], status, last_row, n_end)


def solve_eom(artifact: CompilationArtifact, pars, steps: int, fields_init, derivatives_init, max_err: float = 1e-6, solver: str = "rk4", *,
              dt: float | None = None) -> np.ndarray:  # fmt: skip
    """The reference's ``solve_eom``: one trajectory as a C-contiguous (steps, 5) array with columns phi^0, phi^1, chi^0, chi^1, H;
    row 0 is the initial state, row k the state after k accepted steps.  ``solver`` is ``"rk4"`` (the default, as in the reference)
    or ``"rkf"``.  Extension (keyword-only): ``dt``, a fixed step.  Bit for bit ``solve_eom_batch`` with one trajectory; where that
    trajectory stops early (``status``), the remaining rows are NaN."""
    x = np.asarray(fields_init, dtype=np.float64).reshape(1, -1)
    v = np.asarray(derivatives_init, dtype=np.float64).reshape(1, -1)
    p = np.asarray(pars, dtype=np.float64)
    if p.ndim != 1:
        raise InflatoxShapeError(f"pars must be one parameter row (got shape {p.shape})")
    sol = solve_eom_batch(artifact, p, steps, x, v, max_err, solver, dt=dt)
    return np.ascontiguousarray(sol.states[0])


def grid_points(start_stop, N0: int, N1: int):
    """The field values of an (N0, N1) sweep grid, the sweeps' rule (inflx_coord): x = i * ((stop - start) / N) + start, the end point
    excluded.  Returns (x0 (N0,), x1 (N1,))."""
    ss = np.asarray(start_stop, dtype=np.float64).reshape(2, 2)
    out = []
    for (a, b), n in zip(ss, (N0, N1)):
        spacing = (b - a) / float(n)
        out.append(np.arange(n, dtype=np.float64) * spacing + a)
    return out


def efolds_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, derivatives_init=(0.0, 0.0), max_steps: int = 100_000,
               max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """The number of e-folds at the end of inflation (epsilon_H = 1) from every point of an (N0, N1) grid over ``start_stop``
    ((2, 2): [[x0_start, x0_stop], [x1_start, x1_stop]], the sweeps' layout and coordinate rule), all trajectories starting with the
    velocities ``derivatives_init``.  NaN where inflation did not end within ``max_steps`` accepted steps or the trajectory stopped
    for another reason; ``return_status=True`` returns ``(N_end, status)`` with the (N0, N1) int8 ``STATUS`` codes.  No rows are
    stored (the kernels' final-only mode): memory is O(N0 * N1).

    Accuracy: N_end is linear in epsilon_H across the accepted step in which epsilon_H reaches 1, and near the end of inflation the
    adaptive steps span dN ~ 1e-2; that interpolation, not the integration, sets the error.  On the hyperbolic model at the default
    ``max_err = 1e-8``, N_end is within 6e-4 e-folds of a DOP853 solution with an exact event (2e-5 .. 1e-4 at 1e-10); for more,
    ``solve_eom_batch(..., stop_at_end=True)`` with a small fixed ``dt``.  A point already past the end of inflation (epsilon_H >= 1
    at the start) has N_end = 0."""
    _, _, max_err, _ = _check_common(artifact, max_steps, max_err, solver, None)
    ss, N0, N1, d = _check_grid(start_stop, N0, N1, derivatives_init)
    p = _parameter_row(artifact, pars, "efolds_map takes")
    init = _grid_init(ss, N0, N1, d)
    flags = _native.EOM_STOP_AT_END | _native.EOM_FINAL_ONLY
    _, _, n_end, status, _ = _dylib(artifact).solve_eom(p, init, int(max_steps) + 1, 1, _METHODS[solver], max_err, 0.0, flags)
    n_end = np.where(status == ENDED, n_end, np.nan).reshape(N0, N1)
    status = status.reshape(N0, N1)
    return (n_end, status) if return_status else n_end


def state_at_efolds(artifact: CompilationArtifact, pars, fields_init, derivatives_init, N_target, max_steps: int = 100_000, max_err: float = 1e-8,
                    solver: str = "rkf", *, dt: float | None = None, stop_at_end: bool = True) -> EfoldsState:  # fmt: skip
    """The state of B trajectories where each has made ``N_target`` e-folds (a scalar, or (B,): one target per trajectory), without
    storing rows: memory is O(B).  ``fields_init``, ``derivatives_init``, ``pars``, ``solver``, ``max_err`` and ``dt`` as for
    ``solve_eom_batch``.  A trajectory stops at the first accepted step whose new state has N >= its target (status ``TARGET``) and
    the state is located inside that step: the cubic Hermite interpolant over the step from the states and right-hand sides at its
    two ends -- fourth order, like the steppers --, solved for N = target by a bracketed Newton iteration, N set to the target
    exactly and epsilon_H evaluated at the located state.  A target <= 0 is reached by the initial state.  With ``stop_at_end`` a
    trajectory whose epsilon_H reaches 1 before its target stops there (``ENDED``, ``N_end`` as in ``efolds_map``); one that takes
    ``max_steps`` accepted steps without reaching its target is ``COMPLETE``.  Bad arguments raise before anything runs on the
    device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    x, v = _check_fields(fields_init, derivatives_init)
    B = x.shape[0]
    target = np.asarray(N_target, dtype=np.float64)
    if target.ndim == 0:
        target = np.full(B, float(target))
    if target.shape != (B,):
        raise InflatoxShapeError(f"N_target must be a scalar or have shape ({B},) (got {target.shape})")
    if not np.isfinite(target).all():
        raise ValueError("N_target must be finite")
    p = _pars(artifact, pars, B)
    init = np.concatenate([x, v], axis=1)
    flags = _native.EOM_STOP_AT_END if stop_at_end else 0
    states, t, eps, n_end, status = _dylib(artifact).solve_eom_to_efolds(p, init, np.ascontiguousarray(target), max_steps, _METHODS[solver], max_err, dt or 0.0, flags)
    hit = status == TARGET
    states = np.where(hit[:, None], states, np.nan)
    return EfoldsState(states[:, :5], np.where(hit, t, np.nan), states[:, 5], np.where(hit, eps, np.nan), np.where(status == ENDED, n_end, np.nan), status)


def solve_eom_sampled(artifact: CompilationArtifact, pars, samples, fields_init, derivatives_init, max_steps: int = 100_000, max_err: float = 1e-8,
                      solver: str = "rkf", *, at: str = "N", dt: float | None = None, stop_at_end: bool = True) -> SampledSolution:  # fmt: skip
    """The state of B trajectories at every point of ``samples`` (S,), one list shared by all of them: e-fold counts (``at="N"``) or
    cosmic times (``at="t"``), finite, >= 0 and strictly increasing.  ``fields_init``, ``derivatives_init``, ``pars``, ``solver``,
    ``max_err`` and ``dt`` as for ``solve_eom_batch``; memory is O(B * S) and nothing is rearranged on the host.  The steps are those
    of the ordinary run.  After every accepted step a trajectory emits the samples that step passed, each located inside the step
    with the cubic Hermite interpolant of ``state_at_efolds`` (fourth order, like the steppers): for ``"N"`` the sample's N exactly
    and t interpolated -- bit for bit ``state_at_efolds`` with that target --, for ``"t"`` the sample's t exactly and N
    interpolated; epsilon_H is evaluated at the located state.  A sample equal to 0 is the initial state.  With ``stop_at_end``, in
    the step where epsilon_H reaches 1 only the samples up to that point are emitted (``N_end`` as in ``efolds_map``), the rest are
    NaN and the trajectory is ``ENDED``; one that starts past the end emits only a sample at 0.  ``status`` is ``TARGET`` once all
    S samples are emitted, ``COMPLETE`` when ``max_steps`` accepted steps ran out first (``n_stored`` < S).  Bad arguments raise
    before anything runs on the device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    if at not in ("N", "t"):
        raise ValueError(f"unknown sampling variable {at!r}: choose 'N' or 't'")
    pts = _check_samples(samples, "samples", "samples")
    x, v = _check_fields(fields_init, derivatives_init)
    p = _pars(artifact, pars, x.shape[0])
    init = np.concatenate([x, v], axis=1)
    flags = (_native.EOM_STOP_AT_END if stop_at_end else 0) | (_native.EOM_SAMPLE_T if at == "t" else 0)
    out, n_end, status, n_stored = _dylib(artifact).solve_eom_sampled(p, init, pts, max_steps, _METHODS[solver], max_err, dt or 0.0, flags)
    return SampledSolution(out[:, :5].transpose(2, 0, 1), out[:, 6].T, out[:, 5].T, out[:, 7].T, n_stored, np.where(status == ENDED, n_end, np.nan), status)


def horizon_exit_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, derivatives_init=(0.0, 0.0),
                     max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """The state ``N_star`` e-folds before the end of inflation -- the horizon exit of the pivot scale -- from every point of the
    (N0, N1) grid of ``efolds_map`` (same arguments): ``(state, N_end)`` with ``state`` (N0, N1, 5) = phi^0, phi^1, chi^0, chi^1, H
    at N = N_end - N_star and ``N_end`` (N0, N1) exactly ``efolds_map``'s result.  Two passes, each of O(N0 * N1) memory: the first
    is ``efolds_map``'s run and finds N_end; the second, ``state_at_efolds`` with the target N_end - N_star, runs only the points
    that ended with N_end >= N_star.  It has to be a second pass because N_end is not known before the trajectory has ended, and
    it retraces the first exactly because the integrator is deterministic.  ``state`` is NaN everywhere else;
    ``return_status=True`` adds the (N0, N1) int8 status map: ``TARGET`` where the state was found, ``ENDED_SHORT`` where
    inflation ended after fewer than ``N_star`` e-folds, and the first pass's status (``COMPLETE``: never ended, or a failure)
    otherwise.  The state carries the error of N_end (see ``efolds_map``) times |dphi/dN|."""
    N_star = _check_n_star(N_star)
    n_end, status = efolds_map(artifact, pars, start_stop, N0, N1, derivatives_init, max_steps, max_err, solver, return_status=True)
    N0, N1 = n_end.shape
    status = status.copy().reshape(-1)
    flat_end = n_end.reshape(-1)
    ended = status == ENDED
    status[ended] = ENDED_SHORT
    state = np.full((N0 * N1, 5), np.nan)
    with np.errstate(invalid="ignore"):
        run = np.flatnonzero(ended & (flat_end >= N_star))
    if run.size:
        init = _grid_init(start_stop, N0, N1, np.asarray(derivatives_init, dtype=np.float64).reshape(2))[run]
        got = state_at_efolds(artifact, pars, init[:, :2], init[:, 2:], flat_end[run] - N_star, max_steps, max_err, solver)
        state[run] = got.state
        status[run] = got.status
    state = state.reshape(N0, N1, 5)
    status = status.reshape(N0, N1)
    return (state, n_end, status) if return_status else (state, n_end)


class Kinematics(NamedTuple):
    """What :func:`kinematics` returns, each member of the shape of the states' leading axes and all six views of one (6, ...)
    array.  With sigma_dot^2 = G_ab chi^a chi^b: ``eps_H`` = sigma_dot^2 / (2 H^2), bit for bit the solver's own epsilon_H;
    ``eta_par`` = -sigma_ddot / (H sigma_dot); ``omega`` = Omega / H, the turn rate per e-fold, SIGNED (positive: the trajectory
    turns counter-clockwise in the (phi^0, phi^1) chart) -- the omega >= 0 of ``GeneralisedAL.complete_analysis`` corresponds to
    its absolute value; ``sigma_dot``; ``V_sigma`` and ``V_N``, the gradient of the potential along the velocity and normal to it
    (V_sigma^2 + V_N^2 = |dV|^2)."""

    eps_H: np.ndarray
    eta_par: np.ndarray
    omega: np.ndarray
    sigma_dot: np.ndarray
    V_sigma: np.ndarray
    V_N: np.ndarray


#: the host path reads a strided array in place only up to this many doubles between states: the whole span is uploaded, and beyond
#: the solver's rows (6) and a little slack a contiguous copy of 40 bytes per state is cheaper than the gaps (``sol.states[:, 0]``
#: of (B, steps, 6) rows has 6 * steps doubles between states).  A device tensor is read in place at any uniform stride.
_HOST_MAX_LD = 8


def _state_stride(shape, strides):
    """The distance ``ld``, in elements, between consecutive states of an array of states (..., 5) with ``strides`` in elements, when
    there is one: the last stride is 1 and the leading axes advance uniformly, as in a C-contiguous array (ld = 5) or in the first
    five columns of the solver's (B, steps, 6) rows (ld = 6).  None: the array has to be made contiguous."""
    if strides[-1] != 1:
        return None
    ld = None
    inner = 1  # states one step of the next axis to the left spans
    for size, stride in zip(reversed(shape[:-1]), reversed(strides[:-1])):
        if size > 1:
            if stride <= 0 or stride % inner or (ld is not None and stride != ld * inner):
                return None
            ld = stride // inner
        inner *= size
    if ld is None:
        return 5
    return ld if ld >= 5 else None


def kinematics(artifact: CompilationArtifact, pars, states) -> Kinematics:
    """epsilon_H, eta_parallel, the turn rate and the slopes of the potential at ``states``: (5,), (n, 5) or (B, S, 5) with the
    components phi^0, phi^1, chi^0, chi^1, H -- ``EoMSolution.states``, ``EfoldsState.state``, ``SampledSolution.states``, the
    ``state`` of ``horizon_exit_map`` or states from anywhere else.  ``pars`` is (n_par,), or one row per leading index: (n, n_par)
    for (n, 5) states, (B, n_par) for (B, S, 5) states.  A pointwise pass of one GPU lane per state (csrc/inflx_kinematics.h); the
    kernel is built into ``<artefact>.kinematics`` on first use (``CompilationArtifact.ensure_kinematics``) and the integrator is
    not involved.  A component that is not finite (NaN, +-inf) gives six NaNs, whether or not the model depends on that component --
    the NaN rows after a trajectory stopped stay NaN --, a state at rest
    (sigma_dot = 0) has eps_H = 0, sigma_dot = 0 and NaN elsewhere.

    A numpy array (or anything ``numpy.asarray`` takes) is evaluated in chunks of at most 2^20 states and returns numpy arrays; a
    view with a uniform stride of at most 8 doubles between states, such as ``EoMSolution.states``, is read in place, any other
    is made contiguous first.  A ``torch.float64`` tensor on the GPU takes the
    device path: no byte crosses PCIe and the result is torch tensors, ordered with torch's current stream the way
    ``solve_eom_batch_device`` orders its result.  A tensor whose last stride is 1 and whose row stride is uniform --
    ``solve_eom_batch_device(...).states``, a view of the (B, steps, 6) rows -- is read in place, any other is made contiguous
    first.  Bad arguments raise ``InflatoxShapeError`` / ``ValueError`` before the device is touched."""
    return _state_pass("kinematics", Kinematics, artifact, pars, states)


def _state_pass(what: str, result, artifact: CompilationArtifact, pars, states):
    """``kinematics`` and ``masses``: the pointwise pass ``what`` over ``states``, whose ``len(result._fields)`` planes come back as
    the NamedTuple ``result``.  The object ``<artefact>.<what>`` is built on first use (``CompilationArtifact.ensure_<what>``)."""
    planes = len(result._fields)
    if getattr(artifact, "n_fields", None) != 2:
        raise InflatoxShapeError(f"the {what} require a 2-field model (model has {getattr(artifact, 'n_fields', None)} fields)")
    on_device = type(states).__module__.split(".")[0] == "torch" and bool(getattr(states, "is_cuda", False))
    if on_device:
        import torch

        if states.dtype != torch.float64:
            raise ValueError(f"a device tensor of states must be torch.float64 (got {states.dtype})")
        if (states.device.index or 0) != 0:
            raise ValueError(f"the artefact's handle is on device 0; the states are on {states.device}")
        y = states.detach()
    else:
        try:
            y = np.asarray(states, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("states must be convertible to a float64 array") from None
    shape = tuple(y.shape)
    if len(shape) not in (1, 2, 3) or shape[-1] != 5:
        raise InflatoxShapeError(f"states must have shape (5,), (n, 5) or (B, S, 5) (got {shape})")
    lead = shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    traj_len = shape[1] if len(shape) == 3 else 1
    p = _pars(artifact, pars, lead[0] if lead else 1)
    if on_device:
        out = torch.empty((planes, n), dtype=torch.float64, device=y.device)
        if n:
            ld = _state_stride(shape, tuple(y.stride()))
            if ld is None:
                y, ld = y.contiguous(), 5
            lib = _companion_dylib(artifact, what)
            held = y.untyped_storage().nbytes() - y.storage_offset() * 8  # what the tensor's storage holds from its first element on
            with _side_stream(artifact, y.device, y, out) as stream:
                getattr(lib, what + "_device")(p, y.data_ptr(), held, n, ld, traj_len, out.data_ptr(), out.numel() * 8, stream=stream)
        return result(*out.reshape((planes, *lead)))
    if n == 0:
        return result(*np.empty((planes, *lead)))
    ld = _state_stride(shape, tuple(st // 8 if st % 8 == 0 else 0 for st in y.strides))
    if ld is None or ld > _HOST_MAX_LD:
        y, ld = np.ascontiguousarray(y), 5
    out = getattr(_companion_dylib(artifact, what), what)(p, y, n, ld, traj_len)
    return result(*out.reshape((planes, *lead)))


def turn_rate_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, derivatives_init=(0.0, 0.0),
                  max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` (same arguments) followed by ``kinematics`` at the exit states: ``(kin, state, N_end)`` with ``kin`` the
    :class:`Kinematics` of (N0, N1) arrays at the state ``N_star`` e-folds before the end of inflation from every grid point, and
    ``state`` (N0, N1, 5) and ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s; ``return_status=True`` adds its (N0, N1) status map.
    All six quantities are NaN wherever ``state`` is.  ``kin.eps_H``, ``kin.eta_par`` and ``abs(kin.omega)`` on the trajectories
    are what ``GeneralisedAL.complete_analysis`` over the same grid predicts from the potential under the rapid-turn assumptions:
    this is the map to lay beside it."""
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star, derivatives_init, max_steps, max_err, solver, return_status=True)
    kin = kinematics(artifact, pars, state)
    return (kin, state, n_end, status) if return_status else (kin, state, n_end)


class Masses(NamedTuple):
    """What :func:`masses` returns, each member of the shape of the states' leading axes and all eight views of one (8, ...) array.
    T = chi / sigma_dot and N are the trajectory's own tangent and normal, in :class:`Kinematics`' orientation.  ``V_TT``, ``V_TN``,
    ``V_NN``: the covariant Hesse matrix V_;ab = d_a d_b V - Gamma^c_ab d_c V on (T, T), (T, N) and (N, N); ``ricci``: the Ricci scalar
    R of the field-space metric (2 / r^2 on a sphere, -2 / L^2 on the hyperbolic metric diag(1, L^2 sinh^2(phi / L))); ``eps_H`` and
    ``omega``: :class:`Kinematics`' values, bit for bit; ``M_eff2`` = V_NN / H^2 + eps_H R - omega^2, the entropic mass in the
    sub-horizon equation of Q_s, and ``mu_s2`` = V_NN / H^2 + eps_H R + 3 omega^2, the super-horizon effective entropic mass, both in
    units of H^2."""

    V_TT: np.ndarray
    V_TN: np.ndarray
    V_NN: np.ndarray
    ricci: np.ndarray
    eps_H: np.ndarray
    omega: np.ndarray
    M_eff2: np.ndarray
    mu_s2: np.ndarray


def masses(artifact: CompilationArtifact, pars, states) -> Masses:
    """The covariant Hesse matrix along and across the velocity, the curvature of field space and the entropic masses at ``states``:
    :func:`kinematics`' arguments, shapes ((5,), (n, 5), (B, S, 5)), parameter-row rules and argument checks, and its two paths -- a
    numpy array is evaluated in chunks of at most 2^20 states and returns numpy arrays, a ``torch.float64`` GPU tensor such as
    ``solve_eom_batch_device(...).states`` is read in place and returns tensors.  A pointwise pass of one GPU lane per state
    (csrc/inflx_masses.h); the kernel is built into ``<artefact>.masses`` on first use (``CompilationArtifact.ensure_masses``), and
    neither the integrator nor the kinematics object is involved.  A component that is not finite (NaN, +-inf) gives eight NaNs,
    whether or not the model depends on that component; a state at rest (sigma_dot = 0) has eps_H = 0, a finite ``ricci`` and NaN
    elsewhere."""
    return _state_pass("masses", Masses, artifact, pars, states)


def mass_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, derivatives_init=(0.0, 0.0),
             max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` (same arguments) followed by ``masses`` at the exit states: ``(masses, state, N_end)`` with ``masses`` the
    :class:`Masses` of (N0, N1) arrays at the state ``N_star`` e-folds before the end of inflation from every grid point, and
    ``state`` (N0, N1, 5) and ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s; ``return_status=True`` adds its (N0, N1) status map.
    All eight quantities are NaN wherever ``state`` is."""
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star, derivatives_init, max_steps, max_err, solver, return_status=True)
    mass = masses(artifact, pars, state)
    return (mass, state, n_end, status) if return_status else (mass, state, n_end)


class TransferSolution(NamedTuple):
    """What :func:`transfer_functions` returns.  ``T_SS``, ``T_RS``, ``t``, ``N`` and ``eps_H`` (B, S) and ``states`` (B, S, 5): the
    transfer functions, cosmic time, e-folds, epsilon_H and phi^0, phi^1, chi^0, chi^1, H at every sample -- all views of one
    (S, 10, B) array, trajectory fastest, and NaN for a sample the trajectory did not reach; ``n_stored`` (B,): the samples emitted,
    always the first ``n_stored``; ``N_end``, ``T_SS_end`` and ``T_RS_end`` (B,): N and the transfer functions at epsilon_H = 1 of a
    trajectory that ENDED (``stop_at_end``), NaN otherwise; ``status`` (B,) int8 as for :func:`solve_eom_sampled`."""

    T_SS: np.ndarray
    T_RS: np.ndarray
    t: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    states: np.ndarray
    n_stored: np.ndarray
    N_end: np.ndarray
    T_SS_end: np.ndarray
    T_RS_end: np.ndarray
    status: np.ndarray


def _check_dq_dN(dq_dN, B):
    if dq_dN is None:
        return None
    try:
        d = np.asarray(dq_dN, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("dq_dN must be None, a number or a float64 array") from None
    if d.ndim == 0:
        d = np.full(B, float(d))
    if d.shape != (B,):
        raise InflatoxShapeError(f"dq_dN must be a scalar or have shape ({B},) (got {d.shape})")
    if not np.isfinite(d).all():
        raise ValueError("dq_dN must be finite")
    return np.ascontiguousarray(d)


def transfer_functions(artifact: CompilationArtifact, pars, samples, fields_init, derivatives_init, max_steps: int = 100_000, max_err: float = 1e-8,
                       solver: str = "rkf", *, dq_dN=None, dt: float | None = None, stop_at_end: bool = True) -> TransferSolution:  # fmt: skip
    """The super-horizon transfer functions of B trajectories from their initial states -- horizon exit -- at every e-fold count of
    ``samples`` (S,) since the start: finite, >= 0, strictly increasing, one list shared by all.  ``fields_init``,
    ``derivatives_init``, ``pars``, ``solver``, ``dt``, ``max_steps`` and ``stop_at_end`` as for ``solve_eom_sampled``, and its
    argument checks.  One GPU lane per trajectory integrates the background y = (phi, chi, H, N) together with (q, u, r), cosmic time::

        dq/dt = u,   du/dt = -3 H u - H^2 mu_s2 q,   dr/dt = 2 omega H q sqrt(eps_star / eps_H),   (q, u, r)(0) = (1, H0 dq_dN, 0)

    with ``omega`` the signed turn rate per e-fold of :func:`kinematics`, ``mu_s2`` the super-horizon entropic mass of :func:`masses`
    and eps_star = eps_H at the start, all evaluated by the model inside every Runge-Kutta stage (csrc/inflx_transfer.h).  q =
    Q_s / Q_s(0) is the entropic perturbation; ``T_SS`` = q sqrt(eps_star / eps_H) is S / S_star for S = Q_s / sqrt(2 eps_H), and
    ``T_RS`` = r, where R(N) = R_star + T_RS S_star: 1 + T_RS^2 is the growth of the curvature power after horizon exit for
    uncorrelated modes of equal amplitude.

    Orientation and sign: Q_s is measured along T turned COUNTER-CLOCKWISE in the (phi^0, phi^1) chart.  That is minus the normal N
    of :class:`Kinematics`, the side the trajectory turns towards when omega > 0; with it dR/dN = +2 omega S for the project's
    signed omega.

    ``dq_dN``: d ln Q_s / dN at the start, a scalar or (B,), finite.  None (the default): the slowly decaying root of
    lambda^2 + (3 - eps_star) lambda + mu_s2_star = 0, lambda = [-(3 - eps_star) + sqrt((3 - eps_star)^2 - 4 mu_s2_star)] / 2, and its
    real part -(3 - eps_star) / 2 when the discriminant is negative -- computed on the device from the model at every initial state.

    Steps and samples: the steppers, acceptance rule and statuses are ``solve_eom_sampled``'s, but ``max_err`` bounds the absolute
    Euclidean norm of the error over phi, chi, H, q, u and r (eight components), so an adaptive run takes OTHER steps than
    ``solve_eom_sampled``; with a fixed ``dt`` the background (``states``, ``t``, ``N``, ``eps_H``) is that function's bit for bit.
    Samples are located as there, q and r with the same cubic Hermite interpolant; a sample at 0 has T_SS = 1, T_RS = 0 exactly.
    With ``stop_at_end``, in the step where epsilon_H reaches 1 only the samples up to ``N_end`` are emitted, and ``T_SS_end``,
    ``T_RS_end`` are linear across that step at N_end's own fraction of it (a trajectory that starts past the end: 1 and 0).  A
    trajectory stops (``TARGET``) in the step that emits its last sample; a sample at 0, which the initial state emits, never stops
    it, so ``samples=[0.0]`` asks for the end values alone and runs to the end of inflation (``ENDED``) or ``max_steps``.  As in
    ``solve_eom_sampled``, a step that both passes the last sample and ends inflation (the sample at or before ``N_end``) makes the
    trajectory ``TARGET``, not ``ENDED``: its ``N_end``, ``T_SS_end`` and ``T_RS_end`` are NaN like those of every trajectory that
    is not ``ENDED``; put a sample beyond the end of inflation (or pass ``[0.0]``) where the end values are what is wanted.  A
    trajectory at rest at the start (no direction), or one whose eps_star, omega or mu_s2 there is not finite, is ``NONFINITE`` at
    once with NaN everywhere.  The kernels are built into ``<artefact>.transfer`` on first use
    (``CompilationArtifact.ensure_transfer``).  Bad arguments raise before anything runs on the device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    pts = _check_samples(samples, "samples", "samples")
    x, v = _check_fields(fields_init, derivatives_init)
    p = _pars(artifact, pars, x.shape[0])
    dq = _check_dq_dN(dq_dN, x.shape[0])
    init = np.concatenate([x, v], axis=1)
    flags = _native.EOM_STOP_AT_END if stop_at_end else 0
    out, ends, n_end, status, n_stored = _companion_dylib(artifact, "transfer").transfer_functions(p, init, dq, pts, max_steps, _METHODS[solver], max_err, dt or 0.0, flags)
    ended = status == ENDED
    return TransferSolution(out[:, 8].T, out[:, 9].T, out[:, 6].T, out[:, 5].T, out[:, 7].T, out[:, :5].transpose(2, 0, 1), n_stored,
                            np.where(ended, n_end, np.nan), np.where(ended, ends[:, 0], np.nan), np.where(ended, ends[:, 1], np.nan), status)  # fmt: skip


def transfer_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, derivatives_init=(0.0, 0.0),
                 max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, dq_dN=None, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` (same arguments) followed by ``transfer_functions`` from every exit state to the end of inflation:
    ``((T_RS, T_SS), state, N_end)`` with ``T_RS`` and ``T_SS`` the (N0, N1) end values ``T_RS_end`` and ``T_SS_end`` of the
    trajectory that starts at the fields and velocities of the state ``N_star`` e-folds before the end of inflation from every grid
    point (``samples=[0.0]``, ``stop_at_end``), and ``state`` (N0, N1, 5) and ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s.  The
    second stage takes H again from the Friedmann constraint at the exit state's fields and velocities, not the H of ``state``
    (they differ by the integration error of the first stage).  ``dq_dN``: None, a scalar, or an (N0, N1) array with a value for
    every grid point (finite everywhere, also where no exit state is found).  NaN
    where no exit state was found or the second stage did not reach the end of inflation; ``return_status=True`` adds the (N0, N1)
    status map: ``horizon_exit_map``'s, with the second stage's status (``ENDED`` where the transfer functions are valid) in place
    of ``TARGET``."""
    if dq_dN is not None:
        try:
            n_grid = operator.index(N0) * operator.index(N1)
        except TypeError:
            raise ValueError("N0 and N1 must be integers") from None
        per_point = np.ndim(dq_dN) == 2
        if per_point and np.shape(dq_dN) != (N0, N1):
            raise InflatoxShapeError(f"dq_dN must be a scalar or have shape ({N0}, {N1}) (got {np.shape(dq_dN)})")
        dq_dN = _check_dq_dN(np.reshape(dq_dN, -1) if per_point else dq_dN, max(n_grid, 0) if per_point else 1)
        if not per_point:
            dq_dN = np.full(max(n_grid, 0), dq_dN[0])
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star, derivatives_init, max_steps, max_err, solver, return_status=True)

    def to_the_end(x, v, run):
        tf = transfer_functions(artifact, pars, [0.0], x, v, max_steps, max_err, solver, dq_dN=None if dq_dN is None else dq_dN[run])
        return (tf.T_RS_end, tf.T_SS_end), tf.status

    (t_rs, t_ss), status = _second_stage(state, status, np.int8, [(), ()], to_the_end)
    return ((t_rs, t_ss), state, n_end, status) if return_status else ((t_rs, t_ss), state, n_end)


class PowerSpectra(NamedTuple):
    """What :func:`power_spectra` returns, for B trajectories and K wavenumbers.  ``P_R``, ``P_S`` and ``C_RS`` (B, K): the
    dimensionless power spectra of the curvature perturbation R = H Q_sigma / sigma_dot, of the isocurvature perturbation
    S = H Q_s / sigma_dot and their cross-correlation at the evaluation point; ``k`` (B, K): the comoving wavenumber with a = 1 at the
    trajectory's start, k = H_exit e^N_exit; ``N`` and ``eps_H`` (B, K): the e-fold count since the trajectory's start and epsilon_H at
    the evaluation point (1 at the end of inflation); ``modes`` (B, K, 2, 2) complex: Qt^I_J = a_in sqrt(2 k) Q^I_J there, I the
    Bunch-Davies solution and J the component, both in the order (sigma, s); ``N_end`` (B, K): N since the trajectory's start at
    epsilon_H = 1 of a lane that ``ENDED``, NaN otherwise; ``status`` (B, K) int8.  The values are those of a lane that stopped
    where it was asked to -- ``TARGET`` with ``N_eval``, ``ENDED`` without -- and NaN for every other lane, as in
    :class:`TransferSolution`."""

    P_R: np.ndarray
    P_S: np.ndarray
    C_RS: np.ndarray
    k: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    modes: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


def _check_n_sub(N_sub):
    try:
        N_sub = float(N_sub)
    except (TypeError, ValueError):
        raise ValueError("N_sub must be a number") from None
    if not (math.isfinite(N_sub) and N_sub > 0.0):
        raise ValueError(f"N_sub must be finite and > 0 (got {N_sub})")
    return N_sub


def _check_spectra(artifact, pars, N_exit, fields_init, derivatives_init, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """The argument checks of ``power_spectra`` and ``tensor_spectra``, in their order: (p, n_exit (K,), x, v (B, 2), N_eval, N_sub,
    max_steps, max_err, solver, dt, stop_at_end), what ``_mode_lanes`` takes."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    try:
        n_exit = np.ascontiguousarray(N_exit, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("N_exit must be convertible to a float64 array") from None
    if n_exit.ndim != 1:
        raise InflatoxShapeError(f"N_exit must be one-dimensional (got shape {n_exit.shape})")
    if n_exit.size < 1:
        raise ValueError("N_exit must hold at least one e-fold count")
    N_sub = _check_n_sub(N_sub)
    if not (np.isfinite(n_exit).all() and (n_exit >= N_sub).all()):
        raise ValueError(f"N_exit must be finite and >= N_sub = {N_sub}")
    if N_eval is None:
        if not stop_at_end:
            raise ValueError("N_eval=None evaluates at the end of inflation and needs stop_at_end")
    else:
        try:
            N_eval = float(N_eval)
        except (TypeError, ValueError):
            raise ValueError("N_eval must be None or a number") from None
        if not (math.isfinite(N_eval) and N_eval > n_exit.max()):
            raise ValueError(f"N_eval must be finite and > max(N_exit) = {n_exit.max()} (got {N_eval})")
    x, v = _check_fields(fields_init, derivatives_init)
    B, K = x.shape[0], n_exit.size
    p = _pars(artifact, pars, B)
    return p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end


def _mode_lanes(artifact, tensor, p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """The two stages of ``power_spectra`` (``tensor``: of ``tensor_spectra``, whose first stage is the same call) on checked
    arguments: (out (planes, B K) with NaN for a lane that did not stop where asked, h_exit (B, K), n_exit, lane_start (B K,),
    n_end (B K,), status (B K,))."""
    B, K = x.shape[0], n_exit.size
    h_exit, status, run, lane_start, lane_p, init, kappa, target = _mode_stage1(artifact, p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)
    out = np.full((8 if tensor else 22, B * K), np.nan)
    n_end = np.full(B * K, np.nan)
    if run.size:
        lib = _companion_dylib(artifact, "tensor" if tensor else "modes")
        flags = (_native.EOM_STOP_AT_END if stop_at_end else 0) | (_native.MODES_TENSOR if tensor else 0)
        got, ends, st = lib.mode_spectra(lane_p, init, kappa, target, max_steps, _METHODS[solver], max_err, dt or 0.0, flags)
        _mode_stage2_result(out, n_end, status, run, N_eval, got, ends, st)
    return out, h_exit, n_exit, lane_start, n_end, status


def _mode_stage1(artifact, p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """Stage 1 of ``power_spectra``, ``tensor_spectra`` and ``spectra_evolution`` and the lanes of their stage 2: (h_exit (B, K),
    status (B K,) of stage 1, run -- the lanes b K + j whose start state and exit were found --, lane_start (B K,), and for the lanes
    of ``run``: parameter rows, init (n, 4), kappa (n,), n_target (n,) -- NaN without ``N_eval``)."""
    K = n_exit.size
    B = x.shape[0]
    starts = n_exit - N_sub
    pts, inverse = np.unique(np.concatenate([starts, n_exit]), return_inverse=True)
    bg = solve_eom_sampled(artifact, p, pts, x, v, max_steps, max_err, solver, dt=dt, stop_at_end=stop_at_end)
    start = bg.states[:, inverse[:K], :4]  # (B, K, 4)
    h_exit = bg.states[:, inverse[K:], 4]  # (B, K)
    kappa = h_exit * math.exp(N_sub)
    status = np.repeat(bg.status[:, None], K, axis=1).reshape(-1)
    run = np.flatnonzero((np.isfinite(start).all(axis=2) & np.isfinite(h_exit)).reshape(-1))
    lane_start = np.tile(starts, B)
    target = np.full(run.size, np.nan) if N_eval is None else N_eval - lane_start[run]
    lane_p = p if p.ndim == 1 else np.ascontiguousarray(np.repeat(p, K, axis=0)[run])
    return h_exit, status, run, lane_start, lane_p, np.ascontiguousarray(start.reshape(-1, 4)[run]), np.ascontiguousarray(kappa.reshape(-1)[run]), target


def _mode_stage2_result(out, n_end, status, run, N_eval, got, ends, st):
    """What stage 2 returned for the lanes ``run``, put into the lanes' arrays: the values of a lane that stopped where it was asked
    to, NaN for every other lane."""
    valid = st == (ENDED if N_eval is None else TARGET)
    out[:, run] = np.where(valid[None, :], got, np.nan)
    n_end[run] = np.where(st == ENDED, ends, np.nan)
    status[run] = st


def power_spectra(artifact: CompilationArtifact, pars, N_exit, fields_init, derivatives_init, *, N_eval=None, N_sub: float = 5.0, max_steps: int = 1_000_000,
                  max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True) -> PowerSpectra:  # fmt: skip
    """The curvature and isocurvature power spectra P_R, P_S and their correlation C_RS of B trajectories for K wavenumbers, from
    the Bunch-Davies vacuum: the full linear mode equations along the trajectory (csrc/inflx_modes.h), one GPU lane per (trajectory,
    wavenumber).  ``fields_init``, ``derivatives_init``, ``pars``, ``solver``, ``dt`` and ``max_steps`` as for ``solve_eom_sampled``.

    ``N_exit`` (K,), shared by all trajectories: the e-fold counts since the start at which the modes leave the horizon, k = a H;
    finite and >= ``N_sub``.  ``N_sub`` > 0: how many e-folds before its exit a mode starts, in the vacuum.  ``N_eval``: None -- the
    spectra at the end of inflation, which needs ``stop_at_end`` -- or a scalar e-fold count since the start, > max(N_exit).

    Stage 1 is one ``solve_eom_sampled`` run of the B trajectories at the sorted union of ``N_exit - N_sub`` and ``N_exit``: every
    mode's start state and H at its exit, hence kappa = k / a at its start = H_exit e^N_sub.  Stage 2 runs B K lanes, numbered
    b K + j, each from the fields and velocities of its start state (H is taken again from the Friedmann constraint, as
    ``transfer_map`` documents).  A lane integrates the background together with two complex solutions I = sigma, s of

        dQ_sigma/dt = P_sigma + Omega Q_s,      dP_sigma/dt =  Omega P_s - 3 H P_sigma - (k^2/a^2 + M_sigma_sigma) Q_sigma - M_sigma_s Q_s
        dQ_s/dt     = P_s - Omega Q_sigma,      dP_s/dt     = -Omega P_sigma - 3 H P_s - M_sigma_s Q_sigma - (k^2/a^2 + M_ss) Q_s

    in the frame (T, e_s), e_s = T turned COUNTER-CLOCKWISE in the (phi^0, phi^1) chart -- ``transfer_functions``' direction, minus
    the normal of :class:`Kinematics` --, Omega = omega H the signed turn rate, and M_ab = V_;ab - R_acdb chi^c chi^d + (3 - eps)
    chi_a chi_b + (chi_a V_b + V_a chi_b) / H projected on that frame; M_ss = H^2 (M_eff2 + omega^2) with :class:`Masses`' M_eff2.
    The scaled variables Qt = a_in sqrt(2 k) Q start at Qt^I_J = delta_IJ, Pt^I_J = (-i kappa - H_in) delta_IJ, and

        P_R = kappa^2 sum_I |Qt^I_sigma|^2 / (8 pi^2 eps),  P_S likewise with Qt^I_s,  C_RS = kappa^2 sum_I Re(Qt^I_sigma conj Qt^I_s) / (8 pi^2 eps)

    with eps = epsilon_H at the evaluation point (1 at the end of inflation).  The steppers, acceptance rule and statuses are
    ``solve_eom_sampled``'s; ``max_err`` bounds the absolute Euclidean norm of the error over phi, chi, H, the eight Qt and the eight
    Pt / kappa, all O(1) at the start, so the relative error of a spectrum is about max_err e^(2 N_sub) times the number of steps
    over its own size.  With ``N_eval`` the evaluation point is located as ``state_at_efolds`` locates it, all components with the same
    cubic Hermite interpolant; at the end of inflation the modes are linear across the step that ends it, at N_end's own fraction.
    A lane whose stage 1 samples were not reached keeps stage 1's status and NaN values; a lane at rest at its start is
    ``NONFINITE``.  The kernels are built into ``<artefact>.modes`` on first use (``CompilationArtifact.ensure_modes``).  Bad
    arguments raise before anything runs on the device."""
    args = _check_spectra(artifact, pars, N_exit, fields_init, derivatives_init, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)
    return _power_spectra_result(*_mode_lanes(artifact, False, *args))


def _power_spectra_result(out, h_exit, n_exit, lane_start, n_end, status) -> PowerSpectra:
    """:class:`PowerSpectra` from what ``_mode_lanes`` returns"""
    B, K = h_exit.shape
    out = out.reshape(22, B, K)
    offset = lane_start.reshape(B, K)
    q = out[3:11].reshape(2, 2, 2, B, K)  # [I][J][re, im]
    modes = np.moveaxis(q[:, :, 0] + 1j * q[:, :, 1], (0, 1), (2, 3))
    return PowerSpectra(out[0], out[1], out[2], h_exit * np.exp(n_exit)[None, :], out[19] + offset, out[21], modes, n_end.reshape(B, K) + offset,
                        status.reshape(B, K))  # fmt: skip


def spectrum_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, N_sub: float = 5.0, derivatives_init=(0.0, 0.0),
                 max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` with ``N_star + N_sub`` (otherwise the same arguments) followed by ``power_spectra(N_exit=[N_sub])`` from
    every state found to the end of inflation: ``((P_R, P_S, C_RS), state, N_end)`` with the three (N0, N1) spectra at the end of
    inflation of the mode that leaves the horizon ``N_star`` e-folds before it, from the trajectory of every grid point, and ``state``
    (N0, N1, 5) and ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s at ``N_star + N_sub``: the state at which the mode starts, in
    the vacuum, ``N_sub`` e-folds before its exit.  As in ``transfer_map`` the second stage takes H again from the Friedmann
    constraint.  NaN where no such state was found or the second stage did not reach the end of inflation;
    ``return_status=True`` adds the (N0, N1) status map: ``horizon_exit_map``'s, with the second stage's status (``ENDED`` where the
    spectra are valid) in place of ``TARGET``."""
    N_sub = _check_n_sub(N_sub)
    N_star = _check_n_star(N_star)
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star + N_sub, derivatives_init, max_steps, max_err, solver, return_status=True)

    def to_the_end(x, v, run):
        ps = power_spectra(artifact, pars, [N_sub], x, v, N_sub=N_sub, max_steps=max_steps, max_err=max_err, solver=solver)
        return (ps.P_R[:, 0], ps.P_S[:, 0], ps.C_RS[:, 0]), ps.status[:, 0]

    spectra, status = _second_stage(state, status, np.int8, [()] * 3, to_the_end)
    return (tuple(spectra), state, n_end, status) if return_status else (tuple(spectra), state, n_end)


class SpectraEvolution(NamedTuple):
    """What :func:`spectra_evolution` returns, for B trajectories, K wavenumbers and S samples.  ``P_R``, ``P_S``, ``C_RS`` and
    ``eps_H`` (B, K, S): the spectra of :class:`PowerSpectra` and epsilon_H at every sample; ``N`` (B, K, S): the e-fold count of the
    sample since the trajectory's start -- the sample itself with ``since="start"``, ``N_exit[j]`` plus it with ``since="exit"`` --
    where the lane emitted it; ``k`` (B, K) as in :class:`PowerSpectra`; ``end``: the :class:`PowerSpectra` that ``power_spectra``
    returns for the same arguments, bit for bit (all NaN for a run of samples alone); ``status`` (B, K) int8, ``end.status``.

    A sample a lane never reached is NaN in all five arrays: one before the mode's start, one after the point where the lane
    stopped, every sample of a lane whose stage 1 found no start state.  UNLIKE ``end``, whose values are NaN unless the lane stopped
    where it was asked to, the samples of a lane are kept up to where it stopped WHATEVER its status: a lane whose steps ran out
    (``COMPLETE``) or whose step control failed still returns the samples it passed, and ``status`` tells."""

    P_R: np.ndarray
    P_S: np.ndarray
    C_RS: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    k: np.ndarray
    end: PowerSpectra
    status: np.ndarray


def _check_evolution_samples(samples, since, n_exit, N_eval, N_sub):
    """(samples (S,), shift (K,)): the checked sample list of ``spectra_evolution`` and what a lane of wavenumber j subtracts from it"""
    if since not in ("exit", "start"):
        raise ValueError(f"since must be 'exit' or 'start' (got {since!r})")
    try:
        samples = np.ascontiguousarray(samples, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("samples must be convertible to a float64 array") from None
    if samples.ndim != 1:
        raise InflatoxShapeError(f"samples must be one-dimensional (got shape {samples.shape})")
    if samples.size < 1 or samples.size >= 2**32:
        raise ValueError("samples must hold at least one e-fold count (and fewer than 2^32)")
    if not (np.isfinite(samples).all() and (np.diff(samples) > 0.0).all()):
        raise ValueError("samples must be finite and strictly increasing")
    starts = n_exit - N_sub
    if since == "exit":
        if samples[0] < -N_sub:
            raise ValueError(f"samples since the exit must be >= -N_sub = {-N_sub}: a mode starts N_sub e-folds before its exit (got {samples[0]})")
        shift = np.full(n_exit.size, -N_sub)
    else:
        shift = starts
    if N_eval is not None and not ((samples[-1] - shift) <= (N_eval - starts)).all():
        raise ValueError(f"no sample may lie beyond N_eval = {N_eval} (the last one is {samples[-1]}, since={since!r})")
    return samples, shift


def spectra_evolution(artifact: CompilationArtifact, pars, N_exit, samples, fields_init, derivatives_init, *, since: str = "exit", N_eval=None,
                      N_sub: float = 5.0, max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None,
                      stop_at_end: bool = True) -> SpectraEvolution:  # fmt: skip
    """``power_spectra`` with the spectra of every mode sampled along its evolution: P_R, P_S, C_RS and epsilon_H of the B K lanes at
    the S e-fold counts ``samples`` as well as where the lanes stop, from ONE integration of every lane (csrc/inflx_evolution.h) --
    how a mode's curvature power grows after horizon exit while the trajectory turns, and how its isocurvature power decays.  Every
    argument of ``power_spectra`` means what it means there, and both stages are its own.

    ``samples`` (S,), finite and strictly increasing, shared by all lanes.  ``since="exit"``: e-folds since each mode's own horizon
    exit, each >= ``-N_sub`` (a negative one lies inside the horizon); the lane of wavenumber j is sampled at ``N_exit[j] + samples``
    since the trajectory's start.  ``since="start"``: e-fold counts since the trajectory's start; a sample before a mode's start,
    ``N_exit[j] - N_sub``, comes back NaN for that mode, and a sample exactly there is the vacuum, P_R = P_S = kappa^2 / (8 pi^2 eps),
    C_RS = 0.  ``N_eval=None`` with ``stop_at_end=False`` is allowed here: the lanes stop at their last sample and ``end`` is NaN.  With
    ``N_eval`` given no sample may lie beyond it.

    A lane steps from the end state of each accepted step, never from a located state, so its steps are those of ``power_spectra``'s
    lane: ``end`` is ``power_spectra``'s result bit for bit, and with ``since="start"`` the values at a sample are those of
    ``power_spectra(N_eval=sample)`` bit for bit -- located with the same dense output, epsilon_H from the model at the located
    state.  The step that ends inflation emits the samples up to N_end only.  See :class:`SpectraEvolution` for what a lane that did
    not stop where asked returns.  The kernels are built into ``<artefact>.evolution`` on first use
    (``CompilationArtifact.ensure_evolution``); the modes object is not needed.  Bad arguments raise before anything runs on the
    device."""
    args = _check_spectra(artifact, pars, N_exit, fields_init, derivatives_init, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end or N_eval is None)
    p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, _ = args
    stop_at_end = bool(stop_at_end)
    samples, shift = _check_evolution_samples(samples, since, n_exit, N_eval, N_sub)
    B, K, S = x.shape[0], n_exit.size, samples.size
    h_exit, status, run, lane_start, lane_p, init, kappa, target = _mode_stage1(artifact, p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)
    out = np.full((22, B * K), np.nan)
    n_end = np.full(B * K, np.nan)
    sampled = np.full((S, _native.EV_SAMPLE_PLANES, B * K), np.nan)
    if run.size:
        lib = _companion_dylib(artifact, "evolution")
        got, sm, ends, st = lib.mode_evolution(lane_p, init, kappa, target, np.ascontiguousarray(np.tile(shift, B)[run]), samples, max_steps, _METHODS[solver],
                                               max_err, dt or 0.0, _native.EOM_STOP_AT_END if stop_at_end else 0)  # fmt: skip
        _mode_stage2_result(out, n_end, status, run, N_eval, got, ends, st)
        sampled[:, :, run] = sm
    end = _power_spectra_result(out, h_exit, n_exit, lane_start, n_end, status)
    return _evolution_result(sampled, samples, since, n_exit, end)


def _evolution_result(sampled, samples, since, n_exit, end: PowerSpectra) -> SpectraEvolution:
    """:class:`SpectraEvolution` from the sample planes (S, 6, B K) and ``end``"""
    B, K = end.k.shape
    planes = np.moveaxis(sampled, 0, 2).reshape(sampled.shape[1], B, K, samples.size)  # [plane][b][j][sample]
    where = samples[None, None, :] + (n_exit[None, :, None] if since == "exit" else 0.0)
    n = np.where(np.isnan(planes[3]), np.nan, np.broadcast_to(where, planes[3].shape))
    return SpectraEvolution(planes[0], planes[1], planes[2], n, planes[5], end.k, end, end.status)


def evolution_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, samples, N_star: float = 55.0, N_sub: float = 5.0,
                  derivatives_init=(0.0, 0.0), max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` with ``N_star + N_sub`` (otherwise the same arguments) followed by ``spectra_evolution(N_exit=[N_sub],
    since="exit")`` from every state found to the end of inflation, with ``spectrum_map``'s conventions: ``((P_R, P_S, C_RS), state,
    N_end)`` with the three (N0, N1, S) spectra, at ``samples`` e-folds after its horizon exit, of the mode that leaves the horizon
    ``N_star`` e-folds before the end of inflation, from the trajectory of every grid point; ``state`` and ``N_end`` exactly
    ``horizon_exit_map``'s at ``N_star + N_sub``.  NaN where no such state was found and at a sample the second stage did not reach;
    ``return_status=True`` adds the (N0, N1) status map as ``spectrum_map`` does."""
    N_sub = _check_n_sub(N_sub)
    N_star = _check_n_star(N_star)
    samples, _ = _check_evolution_samples(samples, "exit", np.array([N_sub]), None, N_sub)
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star + N_sub, derivatives_init, max_steps, max_err, solver, return_status=True)

    def to_the_end(x, v, run):
        ev = spectra_evolution(artifact, pars, [N_sub], samples, x, v, since="exit", N_sub=N_sub, max_steps=max_steps, max_err=max_err, solver=solver)
        return (ev.P_R[:, 0], ev.P_S[:, 0], ev.C_RS[:, 0]), ev.status[:, 0]

    spectra, status = _second_stage(state, status, np.int8, [(samples.size,)] * 3, to_the_end)
    return (tuple(spectra), state, n_end, status) if return_status else (tuple(spectra), state, n_end)


def transfer_from_spectra(ev, ref: int):
    """The transfer functions that the sampled spectra ``ev`` (:class:`SpectraEvolution`, or anything with ``P_R``, ``P_S`` and
    ``C_RS`` of shape (..., S)) imply between the sample of index ``ref`` -- taken after horizon exit, marked * -- and every sample:
    with R = R* + T_RS S* and S = T_SS S*,

        T_SS = sqrt(P_S / P_S*),      T_RS = (C_RS / T_SS - C_RS*) / P_S*,

    and the residual P_R - (P_R* + 2 T_RS C_RS* + T_RS^2 P_S*) of the third relation, which the two do not use: how far the evolution
    between the two samples is from that super-horizon form.  Returns ``(T_RS, T_SS, residual)``, each of the spectra's shape; at
    ``ref`` itself T_SS = 1, T_RS = 0 and the residual is 0.  A pure function of its arguments: the measured counterpart of
    ``transfer_functions``' T_RS and T_SS, in the same orientation of e_s."""
    ref = operator.index(ref)
    p_r, p_s, c_rs = (np.asarray(a, dtype=np.float64) for a in (ev.P_R, ev.P_S, ev.C_RS))
    if not (p_r.shape == p_s.shape == c_rs.shape and p_r.ndim >= 1):
        raise InflatoxShapeError(f"P_R, P_S and C_RS must have one shape (..., S) (got {p_r.shape}, {p_s.shape} and {c_rs.shape})")
    if not -p_r.shape[-1] <= ref < p_r.shape[-1]:
        raise ValueError(f"ref must index one of the {p_r.shape[-1]} samples (got {ref})")
    r0, s0, c0 = p_r[..., ref, None], p_s[..., ref, None], c_rs[..., ref, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        t_ss = np.sqrt(p_s / s0)
        t_rs = (c_rs / t_ss - c0) / s0
        residual = p_r - (r0 + 2.0 * t_rs * c0 + t_rs * t_rs * s0)
    return t_rs, t_ss, residual


class TensorSpectra(NamedTuple):
    """What :func:`tensor_spectra` returns, for B trajectories and K wavenumbers.  ``P_T`` (B, K): the dimensionless tensor power
    spectrum, both polarisations, at the evaluation point; ``k``, ``N`` and ``eps_H`` (B, K) as in :class:`PowerSpectra` (``k`` is
    ``power_spectra``'s bit for bit); ``modes`` (B, K) complex: ht = a_in sqrt(2 k) u there, u = h / 2 the canonically normalised
    amplitude of one polarisation; ``N_end`` and ``status`` (B, K) as in :class:`PowerSpectra`.  The values are those of a lane that
    stopped where it was asked to and NaN for every other lane."""

    P_T: np.ndarray
    k: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    modes: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


def tensor_spectra(artifact: CompilationArtifact, pars, N_exit, fields_init, derivatives_init, *, N_eval=None, N_sub: float = 5.0, max_steps: int = 1_000_000,
                   max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True) -> TensorSpectra:  # fmt: skip
    """The tensor power spectrum P_T of B trajectories for K wavenumbers, from the Bunch-Davies vacuum: ``power_spectra``'s tensor
    twin (csrc/inflx_tensor.h), one GPU lane per (trajectory, wavenumber).  The arguments, their checks and their order, the two stages
    and the lane numbering b K + j are ``power_spectra``'s; stage 1 is the identical ``solve_eom_sampled`` call, so ``k`` is
    ``power_spectra``'s bit for bit.  A lane integrates the background together with one complex amplitude

        d ht/dt = pt,      d pt/dt = -3 H pt - (k^2/a^2) ht,      ht = a_in sqrt(2 k) u,   u = h / 2

    in reduced Planck units (those of dH/dt = V - 3 H^2), from ht = 1, pt = -i kappa - H_in, and

        P_T = 2 kappa^2 |ht|^2 / pi^2

    counts both polarisations: 2 H^2 / pi^2 in de Sitter, and r = P_T / P_R = 16 eps in single-field slow roll with ``power_spectra``'s
    P_R.  ``max_err`` bounds the absolute Euclidean norm of the error over phi, chi, H, the two components of ht and the two of
    pt / kappa.  The evaluation point is located and interpolated as in ``power_spectra``.  A lane at rest at its start is NOT an
    error here: a tensor mode needs no direction in field space and P_T does not divide by epsilon_H.  The kernels are built into
    ``<artefact>.tensor`` on first use (``CompilationArtifact.ensure_tensor``).  Bad arguments raise before anything runs on the
    device."""
    args = _check_spectra(artifact, pars, N_exit, fields_init, derivatives_init, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)
    out, h_exit, n_exit, lane_start, n_end, status = _mode_lanes(artifact, True, *args)
    B, K = h_exit.shape
    out = out.reshape(8, B, K)
    offset = lane_start.reshape(B, K)
    return TensorSpectra(out[0], h_exit * np.exp(n_exit)[None, :], out[5] + offset, out[7], out[1] + 1j * out[2], n_end.reshape(B, K) + offset,
                         status.reshape(B, K))  # fmt: skip


class Observables(NamedTuple):
    """What :func:`observables` returns, for B trajectories and K pivots, all (B, K).  ``A_s`` = P_R and ``A_t`` = P_T at the pivot
    wavenumber; ``r`` = P_T / P_R; ``n_s`` = 1 + d ln P_R / d ln k; ``alpha_s`` = d^2 ln P_R / d ln k^2; ``n_t`` = d ln P_T / d ln k;
    ``beta_iso`` = P_S / (P_R + P_S); ``cos_delta`` = C_RS / sqrt(P_R P_S); ``k``: the pivot's comoving wavenumber; ``N_end``: that of
    the pivot's scalar lane; ``status`` int8: the status asked for (``ENDED``, or ``TARGET`` with ``N_eval``) when all six lanes of a
    pivot -- scalar and tensor, at the pivot and ``dN`` on either side -- stopped there, otherwise the largest status code among the
    lanes that did not.  Every value but ``k``, ``N_end`` and ``status`` is NaN unless all six did."""

    A_s: np.ndarray
    A_t: np.ndarray
    r: np.ndarray
    n_s: np.ndarray
    alpha_s: np.ndarray
    n_t: np.ndarray
    beta_iso: np.ndarray
    cos_delta: np.ndarray
    k: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


def log_slopes(k, P):
    """First and second derivative of ln P in ln k at the middle of three points: ``k`` and ``P`` (..., 3), ordered (below, pivot,
    above).  With x = ln k, f = ln P, h1 = x_0 - x_m and h2 = x_p - x_0 -- not equal, because H changes along a trajectory -- the
    Lagrange quadratic through the three points has, at x_0,

        f'  = -h2 / (h1 (h1 + h2)) f_m + (h2 - h1) / (h1 h2) f_0 + h1 / (h2 (h1 + h2)) f_p
        f'' = 2 [f_m / (h1 (h1 + h2)) - f_0 / (h1 h2) + f_p / (h2 (h1 + h2))]

    A pure function of its two arrays.  Returns (f', f'')."""
    w1, w2 = stencil_weights(k)
    f = np.log(np.asarray(P, dtype=np.float64))
    return (w1 * f).sum(axis=-1), (w2 * f).sum(axis=-1)


def stencil_weights(k):
    """The weights (..., 3) of ``log_slopes``' two formulas on (f_m, f_0, f_p), from ``k`` (..., 3): (first, second)."""
    x = np.log(np.asarray(k, dtype=np.float64))
    h1, h2 = x[..., 1] - x[..., 0], x[..., 2] - x[..., 1]
    s = h1 + h2
    first = np.stack([-h2 / (h1 * s), (h2 - h1) / (h1 * h2), h1 / (h2 * s)], axis=-1)
    second = 2.0 * np.stack([1.0 / (h1 * s), -1.0 / (h1 * h2), 1.0 / (h2 * s)], axis=-1)
    return first, second


def observables_from_spectra(scalar, tensor, columns, wanted) -> Observables:
    """The differencing half of :func:`observables`, a pure function: ``scalar`` and ``tensor`` with the members of
    :class:`PowerSpectra` and :class:`TensorSpectra` over (B, U) wavenumbers, ``columns`` (3, K) the columns of (below, pivot, above)
    of every pivot, ``wanted`` the status of a lane that stopped where asked."""
    cols = np.asarray(columns)
    k3 = np.moveaxis(scalar.k[:, cols], 1, -1)  # (B, K, 3)
    pr3, pt3 = np.moveaxis(scalar.P_R[:, cols], 1, -1), np.moveaxis(tensor.P_T[:, cols], 1, -1)
    st6 = np.concatenate([np.moveaxis(scalar.status[:, cols], 1, -1), np.moveaxis(tensor.status[:, cols], 1, -1)], axis=-1)  # (B, K, 6)
    ok = (st6 == wanted).all(axis=-1)
    status = np.where(ok, wanted, np.where(st6 == wanted, -1, st6).max(axis=-1)).astype(np.int8)
    with np.errstate(invalid="ignore", divide="ignore"):
        d1s, d2s = log_slopes(k3, pr3)
        d1t, _ = log_slopes(k3, pt3)
        mid = cols[1]
        p_r, p_s, c_rs, p_t = scalar.P_R[:, mid], scalar.P_S[:, mid], scalar.C_RS[:, mid], tensor.P_T[:, mid]
        values = [p_r, p_t, p_t / p_r, 1.0 + d1s, d2s, d1t, p_s / (p_r + p_s), c_rs / np.sqrt(p_r * p_s)]
    values = [np.where(ok, v, np.nan) for v in values]
    return Observables(*values, scalar.k[:, mid], scalar.N_end[:, mid], status)


def _check_dn(dN):
    try:
        dN = float(dN)
    except (TypeError, ValueError):
        raise ValueError("dN must be a number") from None
    if not (math.isfinite(dN) and dN > 0.0):
        raise ValueError(f"dN must be finite and > 0 (got {dN})")
    return dN


def observables(artifact: CompilationArtifact, pars, N_exit, fields_init, derivatives_init, *, dN: float = 0.5, N_eval=None, N_sub: float = 5.0,
                max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True) -> Observables:  # fmt: skip
    """The scalar amplitude and tilt, the running, the tensor amplitude and tilt, the tensor-to-scalar ratio and the isocurvature
    fraction of B trajectories at K pivots ``N_exit`` (the e-fold counts since the start at which the pivot modes leave the horizon):
    one ``power_spectra`` call and one ``tensor_spectra`` call on the sorted, de-duplicated union of ``N_exit - dN``, ``N_exit`` and
    ``N_exit + dN``, differenced per trajectory in ln k around its own pivot.  The other arguments are ``power_spectra``'s.

    ``dN`` must be finite and > 0, ``N_exit - dN >= N_sub`` (a lower point within a rounding of ``N_sub`` counts as ``N_sub``) and
    ``N_eval > max(N_exit) + dN``; everything raises before the device is touched.

    Per trajectory x = ln k at the three wavenumbers is its own -- k = H_exit e^N_exit, not equally spaced because H changes -- and
    with f = ln P, h1 = x_0 - x_m, h2 = x_p - x_0 the derivatives are those of the Lagrange quadratic through the three points at x_0:

        f'  = -h2 / (h1 (h1 + h2)) f_m + (h2 - h1) / (h1 h2) f_0 + h1 / (h2 (h1 + h2)) f_p
        f'' = 2 [f_m / (h1 (h1 + h2)) - f_0 / (h1 h2) + f_p / (h2 (h1 + h2))]

    (``log_slopes``); n_s = 1 + f'[P_R], alpha_s = f''[P_R], n_t = f'[P_T].  The quadratic's own error is of order dN^2 times the third
    derivative of ln P.  See :class:`Observables` for the members and for ``status``."""
    dN = _check_dn(dN)
    p, n_exit, x, v, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end = _check_spectra(
        artifact, pars, N_exit, fields_init, derivatives_init, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)  # fmt: skip
    below = n_exit - dN
    below = np.where(np.abs(below - N_sub) <= 4.0 * np.finfo(np.float64).eps * max(1.0, N_sub), N_sub, below)
    if not (below >= N_sub).all():
        raise ValueError(f"N_exit - dN must be >= N_sub = {N_sub}")
    if N_eval is not None and not N_eval > n_exit.max() + dN:
        raise ValueError(f"N_eval must be > max(N_exit) + dN = {n_exit.max() + dN} (got {N_eval})")
    pts, inverse = np.unique(np.concatenate([below, n_exit, n_exit + dN]), return_inverse=True)
    kw = dict(N_eval=N_eval, N_sub=N_sub, max_steps=max_steps, max_err=max_err, solver=solver, dt=dt, stop_at_end=stop_at_end)
    scalar = power_spectra(artifact, p, pts, x, v, **kw)
    tensor = tensor_spectra(artifact, p, pts, x, v, **kw)
    return observables_from_spectra(scalar, tensor, inverse.reshape(3, n_exit.size), ENDED if N_eval is None else TARGET)


def observables_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, dN: float = 0.5, N_sub: float = 5.0,
                    derivatives_init=(0.0, 0.0), max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` with ``N_star + N_sub + dN`` (otherwise the same arguments) followed by ``observables(N_exit=[N_sub + dN])``
    from every state found to the end of inflation: ``(obs, state, N_end)`` with ``obs`` the :class:`Observables` of (N0, N1) arrays
    -- n_s, r and the others of the mode that leaves the horizon ``N_star`` e-folds before the end of inflation, from the trajectory of
    every grid point -- and ``state`` (N0, N1, 5) and ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s at ``N_star + N_sub + dN``: the
    state at which the lowest of the three modes starts, in the vacuum.  As in ``spectrum_map`` the second stage takes H again from
    the Friedmann constraint.  NaN where no such state was found or one of the six lanes did not reach the end of inflation;
    ``obs.status`` and, with ``return_status=True``, a fourth member are the (N0, N1) status map: ``horizon_exit_map``'s, with
    ``observables``' status (``ENDED`` where the values are valid) in place of ``TARGET``."""
    N_sub = _check_n_sub(N_sub)
    dN = _check_dn(dN)
    N_star = _check_n_star(N_star)
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star + N_sub + dN, derivatives_init, max_steps, max_err, solver, return_status=True)

    def to_the_end(x, v, run):
        obs = observables(artifact, pars, [N_sub + dN], x, v, dN=dN, N_sub=N_sub, max_steps=max_steps, max_err=max_err, solver=solver)
        return [member[:, 0] for member in obs[:-1]], obs.status[:, 0]

    values, status = _second_stage(state, status, np.int8, [()] * (len(Observables._fields) - 1), to_the_end)
    obs = Observables(*values, status)
    return (obs, state, n_end, status) if return_status else (obs, state, n_end)


# ---- the delta-N expansion -------------------------------------------------------------------------------------------------------
class DeltaN(NamedTuple):
    """What :func:`delta_N` returns, for B stencils.  ``N`` (B,): the centre's e-folds to the surface; ``H_end`` (B,): H on the surface;
    ``N_members`` (B, 3, 3): N of the member at the centre's fields plus ((i - 1) h_0, (j - 1) h_1); ``N_I`` (B, 2) and ``N_IJ``
    (B, 2, 2): the central differences N_,I and N_,IJ; ``N_cov`` (B, 2, 2): N_;IJ = N_,IJ - Gamma^K_IJ N_,K; ``grad2`` (B,):
    G^IJ N_,I N_,J; ``f_NL`` (B,): (5/6) N^;I N^;J N_;IJ / grad2^2; ``P_zeta`` (B,): (H / 2 pi)^2 grad2 with the centre's initial H;
    ``status`` (B,) int16: ``LOCATED`` where all nine members met the surface.  Elsewhere every member from ``N_I`` on is NaN
    (``N_members`` keeps what was found) and ``status`` = s + 16 m (:func:`delta_N_status`): the status s of the lowest member
    m = 3 i + j that failed -- ``COMPLETE``: ``max_steps`` ran out; ``PAST_SURFACE`` -- or, with m = 4, of the centre's search for the
    end of inflation."""

    N: np.ndarray
    H_end: np.ndarray
    N_members: np.ndarray
    N_I: np.ndarray
    N_IJ: np.ndarray
    N_cov: np.ndarray
    grad2: np.ndarray
    f_NL: np.ndarray
    P_zeta: np.ndarray
    status: np.ndarray


_VELOCITY_RULES = {"fixed": _native.DN_FIXED, "slow_roll": _native.DN_SLOW_ROLL}


def delta_N_status(status):
    """(code, member) of a :class:`DeltaN` status: the ``STATUS`` code and the index m = 3 i + j of the member it belongs to (0 for
    ``LOCATED``)."""
    status = np.asarray(status)
    return status % 16, status // 16


def _check_delta_n_options(artifact, h, velocity, max_steps, max_err, solver, dt):
    """The checks ``delta_N`` and ``fnl_map`` share: (h0, h1, max_steps, max_err, dt)."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    try:
        hh = np.asarray(h, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("h must be a number or a pair of numbers") from None
    if hh.shape not in ((), (2,)):
        raise InflatoxShapeError(f"h must be a scalar or a pair (got shape {hh.shape})")
    h0, h1 = (float(v) for v in np.broadcast_to(hh, (2,)))
    if not (math.isfinite(h0) and h0 > 0.0 and math.isfinite(h1) and h1 > 0.0):
        raise ValueError(f"h must be positive and finite (got {h})")
    if velocity not in _VELOCITY_RULES:
        raise ValueError(f"unknown velocity rule {velocity!r}: choose 'fixed' or 'slow_roll' (or pass derivatives_init of shape (B, 3, 3, 2))")
    return h0, h1, max_steps, max_err, dt


def _check_delta_n(artifact, pars, fields_init, derivatives_init, h, velocity, H_end, max_steps, max_err, solver, dt):
    """The argument checks of ``delta_N``: (p, centre (B, 4), vel (B, 9, 2) or None, rule, h0, h1, h_end (B,) or None, max_steps,
    max_err, dt)."""
    h0, h1, max_steps, max_err, dt = _check_delta_n_options(artifact, h, velocity, max_steps, max_err, solver, dt)
    x = np.ascontiguousarray(fields_init, dtype=np.float64)
    if x.ndim != 2 or x.shape[1] != 2:
        raise InflatoxShapeError(f"fields_init must have shape (B, 2) (got {x.shape})")
    B = x.shape[0]
    rule, vel = _VELOCITY_RULES[velocity], None
    if derivatives_init is None:
        if velocity == "fixed":
            raise ValueError("velocity='fixed' needs derivatives_init, the centres' coordinate velocities")
        v = np.zeros_like(x)
    else:
        v = np.ascontiguousarray(derivatives_init, dtype=np.float64)
        if v.ndim == 4:
            if v.shape != (B, 3, 3, 2):
                raise InflatoxShapeError(f"explicit member velocities must have shape ({B}, 3, 3, 2) (got {v.shape})")
            rule, vel = _native.DN_EXPLICIT, np.ascontiguousarray(v.reshape(B, 9, 2))
            v = np.ascontiguousarray(v[:, 1, 1])
        elif v.shape != x.shape:
            raise InflatoxShapeError(f"derivatives_init must have shape ({B}, 2) or ({B}, 3, 3, 2) (got {v.shape})")
    h_end = None
    if H_end is not None:
        try:
            h_end = np.ascontiguousarray(np.broadcast_to(np.asarray(H_end, dtype=np.float64), (B,)))
        except (TypeError, ValueError):
            raise ValueError(f"H_end must be None, a number or an array of shape ({B},)") from None
        if not (np.isfinite(h_end).all() and (h_end > 0.0).all()):
            raise ValueError("H_end must be positive and finite")
    p = _pars(artifact, pars, B)
    return p, np.concatenate([x, v], axis=1), vel, rule, h0, h1, h_end, max_steps, max_err, dt


def _delta_n_result(out, surface, status) -> DeltaN:
    B = out.shape[1]
    n_ij = np.stack([out[11], out[13], out[13], out[12]], axis=1).reshape(B, 2, 2)
    n_cov = np.stack([out[14], out[16], out[16], out[15]], axis=1).reshape(B, 2, 2)
    return DeltaN(out[4], surface[0], out[:9].T.reshape(B, 3, 3), out[9:11].T, n_ij, n_cov, out[17], out[18], out[19], status.astype(np.int16))


def delta_N(artifact: CompilationArtifact, pars, fields_init, derivatives_init=None, *, h=1e-2, velocity: str = "fixed", H_end=None,
            max_steps: int = 1_000_000, max_err: float = 1e-10, solver: str = "rkf", dt: float | None = None) -> DeltaN:  # fmt: skip
    """First and second derivatives of the e-fold count with respect to the initial fields, and the local f_NL of the delta-N
    expansion zeta = N_,I dphi^I + N_,IJ dphi^I dphi^J / 2, around each of the B states ``fields_init`` (B, 2).

    What is differentiated is N(phi; chi(phi)): the e-folds of the trajectory that starts at the fields phi with the velocity that the
    chosen rule gives it there, counted to a surface of uniform density -- the surface H = H_c through the point of the CENTRE's
    trajectory where epsilon_H = 1, or H = ``H_end`` (a number or (B,)) when that is given, which a model whose inflation never ends
    needs.  The rules: ``velocity="fixed"`` gives every member of a stencil the centre's coordinate velocity ``derivatives_init``
    (B, 2); ``"slow_roll"`` gives each, the centre included, chi^a = -G^ab d_b V / (3 H) with H^2 = V / 3 at its own fields
    (``derivatives_init`` is not needed); a ``derivatives_init`` of shape (B, 3, 3, 2) gives every member its velocity explicitly.
    ``"fixed"`` and ``"slow_roll"`` are approximations to the attractor, not the attractor: on a trajectory that has not settled, or
    turns sharply at the start, the derivatives carry the difference, and only explicit velocities taken from neighbouring
    attractor solutions remove it.

    Each stencil is nine trajectories at the offsets (i - 1) ``h``[0], (j - 1) ``h``[1] in field coordinates (``h``: a number or a
    pair), one GPU lane each with the step control of ``solve_eom_batch``; both events are located on the integrator's cubic dense
    output, so N of a member is as accurate as its trajectory (DESIGN.md section 12 has the measured figures: the differences are
    limited by ``max_err``, and by h^2 truncation).  ``pars`` is one row or (B, n): stencil b uses row b for all its members.  Metric
    and connection in the covariant formulas are those at the centre.  The kernels are csrc/inflx_deltan_kernels.hip, built into
    ``<artefact>.deltan`` on first use (``CompilationArtifact.ensure_deltan``).  Returns a :class:`DeltaN`."""
    p, centre, vel, rule, h0, h1, h_end, max_steps, max_err, dt = _check_delta_n(artifact, pars, fields_init, derivatives_init, h, velocity, H_end, max_steps, max_err,
                                                                                 solver, dt)  # fmt: skip
    out, surface, status = _companion_dylib(artifact, "deltan").delta_n(p, centre, vel, rule, h0, h1, h_end, max_steps, _METHODS[solver], max_err, dt or 0.0)
    return _delta_n_result(out, surface, status)


def fnl_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, N_star: float = 55.0, h=1e-2, velocity: str = "fixed",
            derivatives_init=(0.0, 0.0), max_steps: int = 1_000_000, max_err: float = 1e-10, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """``horizon_exit_map`` (same arguments) followed by ``delta_N`` from every exit state to the end of inflation: ``(dn, state,
    N_end)`` with ``dn`` the :class:`DeltaN` of (N0, N1, ...) arrays -- f_NL and the derivatives of N of the mode that leaves the
    horizon ``N_star`` e-folds before the end of inflation, from the trajectory of every grid point -- and ``state`` (N0, N1, 5) and
    ``N_end`` (N0, N1) exactly ``horizon_exit_map``'s.  With ``velocity="fixed"`` the members of a stencil take the exit state's
    velocity; with ``"slow_roll"`` each takes its own slow-roll velocity.  H starts again from the Friedmann constraint.  NaN where no
    exit state was found; ``dn.status`` and, with ``return_status=True``, a fourth member are the (N0, N1) int16 status map:
    ``horizon_exit_map``'s, with ``delta_N``'s status (``LOCATED`` where the values are valid) in place of ``TARGET``."""
    _check_delta_n_options(artifact, h, velocity, max_steps, max_err, solver, None)
    N_star = _check_n_star(N_star)
    state, n_end, status = horizon_exit_map(artifact, pars, start_stop, N0, N1, N_star, derivatives_init, max_steps, max_err, solver, return_status=True)
    shapes = {"N_members": (3, 3), "N_I": (2,), "N_IJ": (2, 2), "N_cov": (2, 2)}

    def to_the_end(x, v, run):
        dn = delta_N(artifact, pars, x, v, h=h, velocity=velocity, max_steps=max_steps, max_err=max_err, solver=solver)
        return dn[:-1], dn.status

    values, status = _second_stage(state, status, np.int16, [shapes.get(name, ()) for name in DeltaN._fields[:-1]], to_the_end)
    dn = DeltaN(*values, status)
    return (dn, state, n_end, status) if return_status else (dn, state, n_end)


class StochasticEfolds(NamedTuple):
    """What :func:`stochastic_efolds` returns, every member (B,) unless noted (``stochastic_map``: (N0, N1) in place of (B,)).
    ``N_mean``, ``N_var``, ``N_m3``, ``N_m4``: the mean and the central moments sum (N - mean)^k / n_ended, k = 2, 3, 4, of the e-fold
    count at the end of inflation, ``N_min`` and ``N_max`` its extremes -- all over the realisations that ENDED inflation, NaN where
    none did; ``n_ended`` their number; ``counts`` (B, 6): the realisations per ``STATUS`` code 0..5; ``N_classical``: the e-fold count
    of the trajectory without noise (NaN where it did not end).  With ``return_samples``, else None: ``N`` (B, R), N_end of a
    realisation that ended inflation and the e-fold count where it stopped otherwise; ``state`` (B, R, 5): phi^0, phi^1, chi^0, chi^1,
    H there; ``status`` (B, R) int8."""

    N_mean: np.ndarray
    N_var: np.ndarray
    N_m3: np.ndarray
    N_m4: np.ndarray
    N_min: np.ndarray
    N_max: np.ndarray
    n_ended: np.ndarray
    counts: np.ndarray
    N_classical: np.ndarray
    N: np.ndarray | None = None
    state: np.ndarray | None = None
    status: np.ndarray | None = None


def _check_stochastic_options(artifact, realisations, seed, noise_scale, dN_max, N_stop, max_steps, max_err, solver, dt):
    """The checks ``stochastic_efolds`` and ``stochastic_map`` share: (R, seed, noise_scale, dN_max, N_stop (NaN: none), max_steps,
    max_err, dt)."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    try:
        R = operator.index(realisations)
        seed = operator.index(seed)
    except TypeError:
        raise ValueError("realisations and seed must be integers") from None
    if R < 1 or R > _native.ST_MAX_REALISATIONS:
        raise ValueError(f"realisations must be in [1, 2^20] (got {R})")
    if seed < 0 or seed >= 2**64:
        raise ValueError(f"seed must be in [0, 2^64) (got {seed})")
    try:
        noise_scale, dN_max = float(noise_scale), float(dN_max)
        N_stop = math.nan if N_stop is None else float(N_stop)
    except (TypeError, ValueError):
        raise ValueError("noise_scale, dN_max and N_stop must be numbers") from None
    if not (math.isfinite(noise_scale) and noise_scale >= 0.0):
        raise ValueError(f"noise_scale must be finite and >= 0 (got {noise_scale})")
    if not dN_max > 0.0:
        raise ValueError(f"dN_max must be positive (got {dN_max})")
    if not math.isnan(N_stop) and not (math.isfinite(N_stop) and N_stop > 0.0):
        raise ValueError(f"N_stop must be None or a positive finite number (got {N_stop})")
    return R, seed, noise_scale, dN_max, N_stop, max_steps, max_err, dt


def _check_streams(streams, B):
    if streams is None:
        return None
    try:
        ids = np.asarray(streams)
        if ids.dtype.kind not in "iu":
            raise TypeError
        if ids.size and (ids.min() < 0 or ids.max() >= 2**32):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("streams must be integers in [0, 2^32)") from None
    if ids.shape != (B,):
        raise InflatoxShapeError(f"streams must have shape ({B},) (got {ids.shape})")
    return np.ascontiguousarray(ids, dtype=np.uint32)


def _stochastic_result(moments, classical, samples, B, R) -> StochasticEfolds:
    counts = moments[6:12].T.astype(np.int64)
    n_classical = np.where(classical[7] == 1.0, classical[0], np.nan)
    extra = (None, None, None)
    if samples is not None:
        lanes = samples.reshape(_native.ST_SAMPLE_PLANES, B, R)
        extra = (lanes[0], np.moveaxis(lanes[1:6], 0, -1), lanes[6].astype(np.int8))
    return StochasticEfolds(moments[0], moments[1], moments[2], moments[3], moments[4], moments[5], counts[:, ENDED], counts, n_classical, *extra)


def _stochastic_run(artifact, p, init, R, ids, seed, noise_scale, dN_max, N_stop, max_steps, max_err, solver, dt, return_samples) -> StochasticEfolds:
    lib = _companion_dylib(artifact, "stochastic")
    method, B = _METHODS[solver], init.shape[0]
    moments, samples = lib.stochastic_efolds(p, init, R, ids, seed, noise_scale, dN_max, N_stop, max_steps, method, max_err, dt or 0.0, return_samples)
    # the classical trajectory: the same entry point with one realisation and no noise (moments: its N_end is the mean and the minimum)
    classical, _ = lib.stochastic_efolds(p, init, 1, ids, seed, 0.0, dN_max, N_stop, max_steps, method, max_err, dt or 0.0)
    return _stochastic_result(moments, classical, samples, B, R)


def stochastic_efolds(artifact: CompilationArtifact, pars, fields_init, derivatives_init, realisations: int, *, seed: int = 0, streams=None,
                      noise_scale: float = 1.0, dN_max: float = 1.0 / 32.0, N_stop: float | None = None, max_steps: int = 1_000_000, max_err: float = 1e-8,
                      solver: str = "rkf", dt: float | None = None, return_samples: bool = False) -> StochasticEfolds:  # fmt: skip
    """The e-fold count to the end of inflation as a random variable: ``realisations`` (R, at most 2^20) solutions of the
    separate-universe Langevin equation from each of the B states ``fields_init``, ``derivatives_init`` (both (B, 2)), one GPU lane
    each, and the moments of N_end over them.  ``pars`` is one row or (B, n): point b uses row b for all its realisations.

    A realisation is the classical trajectory of ``solve_eom_batch(..., stop_at_end=True)`` whose fields take, after every accepted
    step over dN e-folds, the kick  phi^a += s (H / 2 pi) sqrt(dN) e^a_alpha xi^alpha - s^2 (H / 2 pi)^2 dN G^bc Gamma^a_bc / 2  with
    e e^T = G^-1, xi standard normal and s = ``noise_scale``: Brownian motion of variance (H / 2 pi)^2 per e-fold on the field
    manifold (the second term is what makes the law independent of the chart), in the units of ``delta_N``'s P_zeta.  The velocities
    are not kicked -- the momentum noise is neglected -- and H follows the change of the energy density.  Adaptive runs try no step
    longer than ``dN_max`` e-folds (``math.inf`` lifts the bound); a fixed ``dt`` is taken as given.  A realisation ends (``ENDED``)
    where epsilon_H reaches 1, in a step (N_end interpolated as ``efolds_map`` does) or by a kick.  With ``N_stop`` it stops after that
    many e-folds instead (``TARGET``), the last kick covering what is left: the diffusion over a fixed number of e-folds.

    The random numbers are Philox4x32-10 with the key ``seed`` and the counter (accepted-step index, realisation, stream): a
    realisation depends on (seed, stream, r) alone -- not on the batch, on R, or on how the run is split into launches.  ``streams``
    (B,) gives every point a 32-bit stream id; the default is the point's index, so two points of a batch never share their noise.

    The moments are CONDITIONAL on the end of inflation: they are taken over the ``n_ended`` realisations with status ``ENDED``, and
    they are biased -- towards short trajectories -- wherever ``n_ended < R``, for the realisations that ran out of ``max_steps`` or
    failed are the long or the odd ones; ``counts`` says what became of all R.  ``return_samples`` adds every realisation's N, state and
    status.  The kernels are csrc/inflx_stochastic_kernels.hip, built into ``<artefact>.stochastic`` on first use
    (``CompilationArtifact.ensure_stochastic``).  Bad arguments raise before anything runs on the device.  Returns a
    :class:`StochasticEfolds`."""
    R, seed, noise_scale, dN_max, N_stop, max_steps, max_err, dt = _check_stochastic_options(artifact, realisations, seed, noise_scale, dN_max, N_stop, max_steps,
                                                                                             max_err, solver, dt)  # fmt: skip
    x, v = _check_fields(fields_init, derivatives_init)
    B = x.shape[0]
    ids = _check_streams(streams, B)
    p = _pars(artifact, pars, B)
    return _stochastic_run(artifact, p, np.concatenate([x, v], axis=1), R, ids, seed, noise_scale, dN_max, N_stop, max_steps, max_err, solver, dt, bool(return_samples))


def stochastic_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, realisations: int, *, derivatives_init=(0.0, 0.0), seed: int = 0,
                   noise_scale: float = 1.0, dN_max: float = 1.0 / 32.0, N_stop: float | None = None, max_steps: int = 1_000_000, max_err: float = 1e-8,
                   solver: str = "rkf", dt: float | None = None) -> StochasticEfolds:  # fmt: skip
    """``stochastic_efolds`` from every point of an (N0, N1) grid over ``start_stop`` (the sweeps' layout and coordinate rule,
    ``grid_points``), all trajectories starting with the velocities ``derivatives_init``: the same result as (N0, N1) maps (``counts``
    (N0, N1, 6)), the stream of a point its index in the flattened grid.  Beside ``GeneralisedAL.flag_quantum_dif`` over the same grid it
    says what the diffusion does where that flag is set.  It never returns samples."""
    options = _check_stochastic_options(artifact, realisations, seed, noise_scale, dN_max, N_stop, max_steps, max_err, solver, dt)
    ss, N0, N1, d = _check_grid(start_stop, N0, N1, derivatives_init)
    p = _parameter_row(artifact, pars, "stochastic_map takes")
    init = _grid_init(ss, N0, N1, d)
    R, seed, noise_scale, dN_max, N_stop, max_steps, max_err, dt = options
    flat = _stochastic_run(artifact, p, init, R, None, seed, noise_scale, dN_max, N_stop, max_steps, max_err, solver, dt, False)
    return StochasticEfolds(*(a.reshape(N0, N1, *a.shape[1:]) for a in flat[:9]))


class StochasticDistribution(NamedTuple):
    """What :func:`stochastic_distribution` returns (``stochastic_distribution_map``: (N0, N1) in place of (B,)).  ``hist`` (B, bins)
    int64: the realisations that ENDED inflation per bin of the e-fold count N_end; ``below`` and ``above`` (B,): those outside the
    range.  The bin of N is k = floor((N - lo) * (bins / (hi - lo))) in binary64 -- N < lo is below, k >= bins is above, so N = hi is
    above --: that rule is the definition, and ``edges`` (B, bins + 1), lo + k (hi - lo) / bins, are nominal.  ``counts`` (B, 6): the
    realisations per ``STATUS`` code 0..5 and ``n_ended`` = counts[:, ENDED] = below + hist.sum(-1) + above.  ``N_classical``: the
    e-fold count of the trajectory without noise (NaN where it did not end); with ``centre="classical"`` such a point is not run: its
    counts are zero and its edges NaN.  ``realisations``, ``first_realisation`` and ``seed`` are the call's: the realisations are
    first_realisation .. first_realisation + realisations - 1.  Two results of the same edges and seed whose ranges of realisations
    adjoin add up with ``+`` to the result of the call over both ranges, exactly."""

    hist: np.ndarray
    below: np.ndarray
    above: np.ndarray
    edges: np.ndarray
    counts: np.ndarray
    n_ended: np.ndarray
    N_classical: np.ndarray
    realisations: int
    first_realisation: int
    seed: int = 0

    def __add__(self, other):
        if not isinstance(other, StochasticDistribution):
            return NotImplemented
        a, b = (self, other) if self.first_realisation <= other.first_realisation else (other, self)
        if a.seed != b.seed:
            raise ValueError(f"the two distributions have different seeds ({a.seed} and {b.seed})")
        if np.shape(a.edges) != np.shape(b.edges) or not np.array_equal(a.edges, b.edges, equal_nan=True):
            raise ValueError("the two distributions have different edges")
        if a.first_realisation + a.realisations != b.first_realisation:
            raise ValueError(f"the realisations do not adjoin: [{a.first_realisation}, {a.first_realisation + a.realisations}) and "
                             f"[{b.first_realisation}, {b.first_realisation + b.realisations})")  # fmt: skip
        return StochasticDistribution(a.hist + b.hist, a.below + b.below, a.above + b.above, a.edges, a.counts + b.counts, a.n_ended + b.n_ended, a.N_classical,
                                      a.realisations + b.realisations, a.first_realisation, a.seed)  # fmt: skip


def _check_distribution_options(artifact, realisations, bins, centre, seed, first_realisation, lanes_per_point, noise_scale, dN_max, max_steps, max_err, solver, dt):
    """The checks ``stochastic_distribution`` and ``stochastic_distribution_map`` share: (R, bins, seed, first, L (0: the library's
    choice), noise_scale, dN_max, max_steps, max_err, dt)."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    try:
        R, bins, seed, first = operator.index(realisations), operator.index(bins), operator.index(seed), operator.index(first_realisation)
        L = 0 if lanes_per_point is None else operator.index(lanes_per_point)
    except TypeError:
        raise ValueError("realisations, bins, seed, first_realisation and lanes_per_point must be integers") from None
    if R < 1 or R > _native.PD_MAX_REALISATIONS:
        raise ValueError(f"realisations must be in [1, 2^32 - 1] (got {R})")
    if bins < 1 or bins > _native.PD_MAX_BINS:
        raise ValueError(f"bins must be in [1, 2^20] (got {bins})")
    if seed < 0 or seed >= 2**64:
        raise ValueError(f"seed must be in [0, 2^64) (got {seed})")
    if first < 0 or first + R > 2**32:
        raise ValueError(f"first_realisation must be >= 0 and first_realisation + realisations at most 2^32 (got {first} + {R})")
    if lanes_per_point is not None and (L < 64 or L % 64 or L > _native.PD_MAX_LANES_PER_POINT):
        raise ValueError(f"lanes_per_point must be None or a multiple of 64 in [64, 2^20] (got {L})")
    if centre not in (None, "classical"):
        raise ValueError(f'centre must be None or "classical" (got {centre!r})')
    try:
        noise_scale, dN_max = float(noise_scale), float(dN_max)
    except (TypeError, ValueError):
        raise ValueError("noise_scale and dN_max must be numbers") from None
    if not (math.isfinite(noise_scale) and noise_scale >= 0.0):
        raise ValueError(f"noise_scale must be finite and >= 0 (got {noise_scale})")
    if not dN_max > 0.0:
        raise ValueError(f"dN_max must be positive (got {dN_max})")
    return R, bins, seed, first, L, noise_scale, dN_max, max_steps, max_err, dt


def _check_n_range(N_range, B):
    """``N_range`` as (1, 2) or (B, 2): finite, hi above lo"""
    try:
        r = np.array(N_range, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("N_range must be numbers") from None
    if r.shape == (2,):
        r = r.reshape(1, 2)
    if r.ndim != 2 or r.shape[1] != 2 or r.shape[0] not in (1, B):
        raise InflatoxShapeError(f"N_range must be (lo, hi) or have shape ({B}, 2) (got {r.shape})")
    with np.errstate(over="ignore", invalid="ignore"):
        finite = np.all(np.isfinite(r)) and np.all(np.isfinite(r[:, 1] - r[:, 0]))
    if not finite:
        raise ValueError("N_range must be finite (and so its width)")
    if not np.all(r[:, 1] > r[:, 0]):
        raise ValueError("N_range is empty: hi must be above lo")
    return r


def _distribution_run(artifact, p, init, ranges, ids, centre, options, solver) -> StochasticDistribution:
    R, bins, seed, first, L, noise_scale, dN_max, max_steps, max_err, dt = options
    lib = _companion_dylib(artifact, "stochastic", "distribution")
    method, B = _METHODS[solver], init.shape[0]
    ids = np.arange(B, dtype=np.uint32) if ids is None else ids
    # the classical trajectory as _stochastic_run finds it: one realisation and no noise (moments: its N_end is the mean)
    classical, _ = lib.stochastic_efolds(p, init, 1, ids, seed, 0.0, dN_max, math.nan, max_steps, method, max_err, dt or 0.0)
    n_classical = np.where(classical[6 + ENDED] == 1.0, classical[0], np.nan)
    ranges = np.broadcast_to(ranges, (B, 2)).copy()
    run = np.ones(B, dtype=bool)
    if centre == "classical":
        run = np.isfinite(n_classical)
        ranges = ranges + np.where(run, n_classical, np.nan)[:, None]
        if not np.all(ranges[run, 1] > ranges[run, 0]):
            raise ValueError("N_range is empty beside the classical e-fold count: hi must be above lo")
    hist = np.zeros((B, bins + 2), dtype=np.int64)
    counts = np.zeros((B, 6), dtype=np.int64)
    if run.any():
        rows = p if p.ndim == 1 else np.ascontiguousarray(p[run])
        h, c = lib.stochastic_distribution(rows, np.ascontiguousarray(init[run]), R, np.ascontiguousarray(ids[run]), seed, first, L, noise_scale, dN_max, max_steps,
                                           method, max_err, dt or 0.0, bins, np.ascontiguousarray(ranges[run]))  # fmt: skip
        hist[run], counts[run] = h, c
    edges = ranges[:, :1] + np.arange(bins + 1, dtype=np.float64) * ((ranges[:, 1:] - ranges[:, :1]) / bins)
    return StochasticDistribution(hist[:, 1:-1], hist[:, 0], hist[:, -1], edges, counts, counts[:, ENDED], n_classical, R, first, seed)


def stochastic_distribution(artifact: CompilationArtifact, pars, fields_init, derivatives_init, realisations: int, bins: int, N_range, *, centre: str | None = None,
                            seed: int = 0, streams=None, first_realisation: int = 0, lanes_per_point: int | None = None, noise_scale: float = 1.0,
                            dN_max: float = 1.0 / 32.0, max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf",
                            dt: float | None = None) -> StochasticDistribution:  # fmt: skip
    """The distribution P(N) of the e-fold count to the end of inflation, as a histogram per point: ``realisations`` (R, up to
    2^32 - 1 -- no chunking is needed) solutions of ``stochastic_efolds``' Langevin equation from each of the B states ``fields_init``,
    ``derivatives_init`` (both (B, 2)), binned on the GPU the moment they end.  The tail of P(N), which four moments do not show, sets
    the abundance of primordial black holes in stochastic delta-N.

    Every point has ``lanes_per_point`` GPU lanes (a multiple of 64; None: the smallest multiple of 64 that is >= R, but no more than
    an equal share, floor(2^20 / B), of the 2^20 lanes of one pass, and no less than 64: few points get many lanes each).  A lane runs
    a realisation to its stop, counts it, draws the point's next ticket and starts that realisation afresh from the point's initial
    state; no lane idles while its point has tickets, and memory is O(lanes + bins), not O(R).  Realisation r is the one
    ``stochastic_efolds`` runs for the same ``seed``, stream and r -- its random numbers are keyed by (seed; its own accepted-step
    index, r, stream) -- and counts are integers, so the result does not depend on ``lanes_per_point`` or on scheduling, bit for
    bit; it is the binning of ``stochastic_efolds(..., return_samples=True).N`` where that call is possible.

    ``N_range`` is (lo, hi) for all points or (B, 2); with ``centre="classical"`` it holds offsets from every point's classical
    e-fold count (one run without noise, ``N_classical``), and a point whose classical run does not end is not run: zero counts, NaN
    edges.  ``bins`` in [1, 2^20]; the bin rule is :class:`StochasticDistribution`'s.  The realisations are ``first_realisation`` ..
    ``first_realisation + R - 1`` (at most 2^32 in all), so that calls over adjoining ranges add up (``+``) to the call over their
    union.  ``streams``, ``noise_scale``, ``dN_max``, ``max_steps``, ``max_err``, ``solver`` and ``dt`` are ``stochastic_efolds``';
    there is no ``N_stop`` (every N would be the same).  Only realisations that ENDED inflation are binned: ``counts`` says what became
    of all R, and a realisation that ran out of ``max_steps`` counts as ``COMPLETE`` -- where ``n_ended < R`` the histogram misses the
    long realisations, which are the tail.  The kernels are csrc/inflx_distribution_kernels.hip, built into
    ``<artefact>.distribution`` on first use (``CompilationArtifact.ensure_distribution``).  Bad arguments raise before anything
    runs on the device."""
    options = _check_distribution_options(artifact, realisations, bins, centre, seed, first_realisation, lanes_per_point, noise_scale, dN_max, max_steps, max_err,
                                          solver, dt)  # fmt: skip
    x, v = _check_fields(fields_init, derivatives_init)
    B = x.shape[0]
    ids = _check_streams(streams, B)
    p = _pars(artifact, pars, B)
    ranges = _check_n_range(N_range, B)
    return _distribution_run(artifact, p, np.concatenate([x, v], axis=1), ranges, ids, centre, options, solver)


def stochastic_distribution_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, realisations: int, bins: int, N_range, *,
                                centre: str | None = "classical", derivatives_init=(0.0, 0.0), seed: int = 0, first_realisation: int = 0,
                                lanes_per_point: int | None = None, noise_scale: float = 1.0, dN_max: float = 1.0 / 32.0, max_steps: int = 1_000_000,
                                max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None) -> StochasticDistribution:  # fmt: skip
    """``stochastic_distribution`` from every point of an (N0, N1) grid over ``start_stop`` (the sweeps' layout and coordinate rule,
    ``grid_points``), all trajectories starting with the velocities ``derivatives_init``: the same result as (N0, N1, ...) maps
    (``hist`` (N0, N1, bins), ``edges`` (N0, N1, bins + 1), ``counts`` (N0, N1, 6)), the stream of a point its index in the flattened
    grid.  ``N_range`` is (lo, hi) or (N0 * N1, 2) and by default holds offsets from every point's classical e-fold count
    (``centre="classical"``): one range then serves a grid whose points are at very different distances from the end of inflation.
    A grid point whose classical run does not end has zero counts and NaN edges."""
    options = _check_distribution_options(artifact, realisations, bins, centre, seed, first_realisation, lanes_per_point, noise_scale, dN_max, max_steps, max_err,
                                          solver, dt)  # fmt: skip
    ss, N0, N1, d = _check_grid(start_stop, N0, N1, derivatives_init)
    p = _parameter_row(artifact, pars, "stochastic_distribution_map takes")
    ranges = _check_n_range(N_range, N0 * N1)
    init = _grid_init(ss, N0, N1, d)
    flat = _distribution_run(artifact, p, init, ranges, None, centre, options, solver)
    return StochasticDistribution(*(a.reshape(N0, N1, *a.shape[1:]) for a in flat[:7]), *flat[7:])


def _distribution_width(d: StochasticDistribution):
    bins = d.hist.shape[-1]
    return (d.edges[..., -1] - d.edges[..., 0]) / bins


def distribution_pdf(d: StochasticDistribution) -> np.ndarray:
    """The density of N_end over the realisations that ended inflation, hist / (n_ended width), same shape as ``hist``: it integrates
    over the range to the share of them that fell inside it.  NaN where none ended."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return d.hist / (np.asarray(d.n_ended, dtype=np.float64) * _distribution_width(d))[..., None]


def distribution_survival(d: StochasticDistribution) -> np.ndarray:
    """P(N_end >= edge) at every edge, (sum of hist from that bin on + above) / n_ended, shape of ``edges``: ratios of exact integers,
    one rounding each.  NaN where none ended."""
    tail = np.concatenate([np.cumsum(d.hist[..., ::-1], axis=-1)[..., ::-1], np.zeros_like(d.hist[..., :1])], axis=-1) + np.asarray(d.above)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return tail / np.asarray(d.n_ended, dtype=np.float64)[..., None]


def distribution_mean(d: StochasticDistribution) -> np.ndarray:
    """The mean of N_end FROM THE BINS: every count inside the range at the midpoint of its bin, ``below`` and ``above`` left out.  It is
    within half a bin width of the mean of the realisations inside the range, not the mean of all of them (``stochastic_efolds`` has
    that, for R <= 2^20).  NaN where no realisation fell inside."""
    mid = 0.5 * (d.edges[..., :-1] + d.edges[..., 1:])
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d.hist * mid).sum(axis=-1) / d.hist.sum(axis=-1)


def distribution_tail_rate(d: StochasticDistribution, N_from):
    """The rate Lambda of an exponential tail P(N) ~ exp(-Lambda N) above ``N_from``, and its standard error: (rate, stderr), shaped
    like ``n_ended``.  The tail starts at the first edge e at or after ``N_from`` (a number, or one per point); with the counts above
    it at the midpoints of their bins and the ``above`` realisations censored at hi, the maximum-likelihood rate is

        Lambda = n_in / (sum_k hist_k (mid_k - e) + above (hi - e)),        n_in = sum_k hist_k over the bins from e on,

    and its standard error Lambda / sqrt(n_in).  The midpoints bias it by (Lambda width)^2 / 12, relative.  NaN where no count lies
    above e inside the range, or ``N_from`` is above the range."""
    bins = d.hist.shape[-1]
    hist = d.hist.reshape(-1, bins)
    edges = d.edges.reshape(-1, bins + 1)
    above = np.asarray(d.above).reshape(-1)
    start = np.broadcast_to(np.asarray(N_from, dtype=np.float64), np.shape(d.n_ended)).reshape(-1)
    rate = np.full(hist.shape[0], np.nan)
    err = np.full(hist.shape[0], np.nan)
    for b in range(hist.shape[0]):
        if not (np.isfinite(edges[b, 0]) and start[b] <= edges[b, -1]):
            continue
        k = int(np.searchsorted(edges[b], start[b], side="left"))
        e = edges[b, k]
        mid = 0.5 * (edges[b, k:-1] + edges[b, k + 1 :])
        n_in = int(hist[b, k:].sum())
        exposure = float((hist[b, k:] * (mid - e)).sum() + above[b] * (edges[b, -1] - e))
        if n_in > 0 and exposure > 0.0:
            rate[b] = n_in / exposure
            err[b] = rate[b] / math.sqrt(n_in)
    shape = np.shape(d.n_ended)
    return rate.reshape(shape), err.reshape(shape)


# ---- horizon crossings: states at given comoving wavenumbers, the pivot scale ------------------------------------------------------
#: ``power_spectra_at_k``, ``tensor_spectra_at_k`` and ``observables_at_k`` only (no kernel status): the mode was outside the horizon
#: at the trajectory's start, or left it fewer than ``N_sub`` e-folds after the start
OUTSIDE_AT_START = 9
STATUS[OUTSIDE_AT_START] = "the mode was outside the horizon at the start, or left it fewer than N_sub e-folds later (power_spectra_at_k)"

#: the constants of ``reheating_offset``: 1 / Mpc = hbar c / Mpc and 1 K = k_B K in GeV (CODATA 2018, IAU 2015: 6.39493e-39 and
#: 8.617333e-14), the CMB temperature today in K, the entropy degrees of freedom today
MPC_INV_GEV = 1.973269804e-16 / 3.0856775814913673e22
KELVIN_GEV = 8.617333262e-14
T_CMB_K = 2.7255
GS_TODAY = 43.0 / 11.0


class CrossingSolution(NamedTuple):
    """What :func:`horizon_crossings` returns, for B trajectories and S wavenumbers.  ``states`` (B, S, 5): phi^0, phi^1, chi^0, chi^1,
    H where ln(a H) reaches ``offset + ln_k[j]``; ``N``, ``t`` and ``eps_H`` (B, S): e-folds, cosmic time and epsilon_H there -- views
    of one (S, 8, B) array, trajectory fastest; ``ln_aH`` (B, S): N + ln H of the located state, the target up to the residual of the
    root search; all five are NaN for a crossing that was not emitted.  ``n_before`` (B,): the targets below ln H_0, whose modes were
    outside the horizon before the start; ``n_stored`` (B,): the crossings emitted, always j = ``n_before`` .. ``n_before + n_stored
    - 1``; ``N_end`` (B,): N at epsilon_H = 1 of a trajectory that ENDED (``stop_at_end``; ``efolds_map``'s linear rule), NaN
    otherwise; ``status`` (B,) int8: ``TARGET`` when every crossing at or after the start was emitted."""

    states: np.ndarray
    N: np.ndarray
    t: np.ndarray
    eps_H: np.ndarray
    ln_aH: np.ndarray
    n_stored: np.ndarray
    n_before: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


class InflationEnd(NamedTuple):
    """What :func:`inflation_end` returns.  ``state`` (B, 5): phi^0, phi^1, chi^0, chi^1, H where epsilon_H = 1 on the dense output;
    ``N_end``, ``t_end`` and ``eps_H`` (B,): e-folds, cosmic time and epsilon_H there (1 up to the root search's bracket) -- all NaN
    unless ``status`` (B,) int8 is ``ENDED``."""

    state: np.ndarray
    N_end: np.ndarray
    t_end: np.ndarray
    eps_H: np.ndarray
    status: np.ndarray


class ExitPoints(NamedTuple):
    """The second value of :func:`power_spectra_at_k` and :func:`tensor_spectra_at_k`: ``ln_k`` (K,) as requested (without the
    offset) and ``N_exit`` (B, K), the e-fold count at which every trajectory's ln(a H) crosses it -- NaN where it does not."""

    ln_k: np.ndarray
    N_exit: np.ndarray


def _check_ln_k(ln_k):
    return _check_samples(ln_k, "ln_k", "wavenumbers", negative=True)


def _check_offset(offset, B):
    if offset is None:
        return np.zeros(B)
    try:
        off = np.asarray(offset, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("offset must be None, a number or an array of numbers") from None
    if off.ndim == 0:
        off = np.full(B, float(off))
    if off.shape != (B,):
        raise InflatoxShapeError(f"offset must be None, a scalar or have shape ({B},) (got {off.shape})")
    if not np.isfinite(off).all():
        raise ValueError("offset must be finite")
    return np.ascontiguousarray(off)


def _crossing_dylib(artifact):
    return _companion_dylib(artifact, "crossing")


def horizon_crossings(artifact: CompilationArtifact, pars, ln_k, fields_init, derivatives_init, *, offset=None, max_steps: int = 100_000,
                      max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True) -> CrossingSolution:  # fmt: skip
    """The state of B trajectories where the comoving Hubble scale ln(a H) = N + ln H reaches every point of ``ln_k`` (S,), one list
    shared by all of them: the horizon exits of the comoving wavenumbers k = e^ln_k, in the solver's own units -- 3 H^2 = rho, reduced
    Planck mass 1, a = 1 at the trajectory's start, so that ln(a H) starts at ln H_0.  ``ln_k`` is finite and strictly increasing and
    may be negative; ``offset`` (None, a scalar or (B,)) is added to it per trajectory: the targets of trajectory b are
    ``offset[b] + ln_k[j]``.  The other arguments are ``solve_eom_sampled``'s, and so are the steps: a trajectory goes on from every
    accepted step's end state.

    Crossing j is emitted from the first accepted step whose end state has ln(a H) >= its target, at the theta in (0, 1] where the
    cubic Hermite interpolants of N and H over the step (``state_at_efolds``' dense output) have N(theta) + ln H(theta) = target:
    Newton's iteration inside a bracket that every iterate tightens, an iterate that leaves the bracket or is not finite replaced by
    the midpoint, at most 64 iterations, stopping at 1e-15 in theta.  All components come from the interpolant at theta, epsilon_H from
    the model there; neither N nor H is overwritten, so ``ln_aH`` differs from the target by what the stopping rule leaves.  A target
    below ln H_0 is not emitted -- the mode was outside the horizon before the start -- and counted in ``n_before``; one equal to it
    is the initial state.  With ``stop_at_end`` the step that ends inflation emits only the crossings whose N is <= ``N_end``; without
    it ln(a H) may fall again, and the first step whose end state reaches the target still defines the crossing.  ``status`` is
    ``TARGET`` once every crossing at or after the start is emitted, ``ENDED`` or ``COMPLETE`` otherwise, ``NONFINITE`` for a located
    state that is not finite.  The kernels are built into ``<artefact>.crossing`` on first use
    (``CompilationArtifact.ensure_crossing``).  Bad arguments raise before anything runs on the device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    pts = _check_ln_k(ln_k)
    x, v = _check_fields(fields_init, derivatives_init)
    B = x.shape[0]
    off = _check_offset(offset, B)
    p = _pars(artifact, pars, B)
    init = np.concatenate([x, v], axis=1)
    flags = _native.EOM_STOP_AT_END if stop_at_end else 0
    out, n_end, status, n_stored, n_before = _crossing_dylib(artifact).solve_eom_crossings(p, init, off, pts, max_steps, _METHODS[solver], max_err, dt or 0.0, flags)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln_ah = out[:, 5].T + np.log(out[:, 4].T)
    return CrossingSolution(out[:, :5].transpose(2, 0, 1), out[:, 5].T, out[:, 6].T, out[:, 7].T, ln_ah, n_stored, n_before,
                            np.where(status == ENDED, n_end, np.nan), status)  # fmt: skip


def inflation_end(artifact: CompilationArtifact, pars, fields_init, derivatives_init, *, max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf",
                  dt: float | None = None) -> InflationEnd:  # fmt: skip
    """The end of inflation of B trajectories as a state: a trajectory stops in the first accepted step whose end state has
    epsilon_H >= 1, and the point where epsilon_H = 1 is located on that step's cubic Hermite interpolant by the Illinois iteration that
    ``delta_N``'s centres use, epsilon_H evaluated through the model at every iterate.  The whole located state is returned, so H_end
    and N_end are read off the same point.  This ``N_end`` is accurate to the dense output's order; ``efolds_map``'s and
    ``solve_eom_sampled``'s are linear in epsilon_H across the step, and the two differ at second order in the step (nothing is pinned
    between them).  A trajectory that starts at or past the end ends at its initial state, ``N_end`` = 0.  ``status`` is ``ENDED`` where
    the end was found and ``COMPLETE`` where ``max_steps`` accepted steps ran out first.  The kernels are those of
    ``<artefact>.crossing``.  Bad arguments raise before anything runs on the device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    x, v = _check_fields(fields_init, derivatives_init)
    p = _pars(artifact, pars, x.shape[0])
    init = np.concatenate([x, v], axis=1)
    states, t, eps, status = _crossing_dylib(artifact).inflation_end(p, init, max_steps, _METHODS[solver], max_err, dt or 0.0)
    hit = status == ENDED
    states = np.where(hit[:, None], states, np.nan)
    return InflationEnd(states[:, :5], states[:, 5], np.where(hit, t, np.nan), np.where(hit, eps, np.nan), status)


def _check_at_k(artifact, pars, ln_k, fields_init, derivatives_init, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """The argument checks of the ``*_at_k`` calls: (p, ln_k (K,), x, v (B, 2), offset (B,), N_eval, N_sub, max_steps, max_err, dt)."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    pts = _check_ln_k(ln_k)
    N_sub = _check_n_sub(N_sub)
    if N_eval is None:
        if not stop_at_end:
            raise ValueError("N_eval=None evaluates at the end of inflation and needs stop_at_end")
    else:
        try:
            N_eval = float(N_eval)
        except (TypeError, ValueError):
            raise ValueError("N_eval must be None or a number") from None
        if not (math.isfinite(N_eval) and N_eval > N_sub):
            raise ValueError(f"N_eval must be finite and > N_sub = {N_sub} (got {N_eval})")
    x, v = _check_fields(fields_init, derivatives_init)
    off = _check_offset(offset, x.shape[0])
    p = _pars(artifact, pars, x.shape[0])
    return p, pts, x, v, off, N_eval, N_sub, max_steps, max_err, dt


def _mode_lanes_at_k(artifact, tensor, p, pts, x, v, off, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """``_mode_lanes`` with every trajectory's own exits: (out (planes, B K), h_exit (B, K), n_exit (B, K), lane_start (B K,),
    n_end (B K,), status (B K,))."""
    B, K = x.shape[0], pts.size
    cr = horizon_crossings(artifact, p, pts, x, v, offset=off, max_steps=max_steps, max_err=max_err, solver=solver, dt=dt, stop_at_end=stop_at_end)
    n_exit = np.array(cr.N)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(n_exit) & (n_exit >= N_sub)
        if N_eval is not None and (n_exit[inside] >= N_eval).any():
            raise ValueError(f"N_eval must be > every located N_exit (the largest is {n_exit[inside].max()}, N_eval = {N_eval})")
    # a crossing that was not emitted keeps its trajectory's status, unless the mode was outside at the start (or too close to it)
    emitted = np.arange(K)[None, :] >= cr.n_before[:, None]
    status = np.where(emitted & ~np.isfinite(n_exit), cr.status[:, None], OUTSIDE_AT_START).astype(np.int8).reshape(-1)
    lanes = np.flatnonzero(inside.reshape(-1))
    b_of = lanes // K
    exits = n_exit.reshape(-1)[lanes]
    starts = exits - N_sub
    lane_start = np.full(B * K, np.nan)
    lane_start[lanes] = starts
    h_exit = np.full(B * K, np.nan)
    out = np.full((8 if tensor else 22, B * K), np.nan)
    n_end = np.full(B * K, np.nan)
    if lanes.size:
        rows = p if p.ndim == 1 else p[b_of]
        n = lanes.size
        both = state_at_efolds(artifact, rows if p.ndim == 1 else np.concatenate([rows, rows]), np.concatenate([x[b_of], x[b_of]]), np.concatenate([v[b_of], v[b_of]]),
                               np.concatenate([starts, exits]), max_steps, max_err, solver, dt=dt, stop_at_end=stop_at_end)  # fmt: skip
        start, h = both.state[:n, :4], both.state[n:, 4]
        h_exit[lanes] = h
        found = np.isfinite(start).all(axis=1) & np.isfinite(h)
        status[lanes] = np.where(found, TARGET, np.where(both.status[:n] != TARGET, both.status[:n], both.status[n:]))
        run = lanes[found]
        if run.size:
            lib = _companion_dylib(artifact, "tensor" if tensor else "modes")
            flags = (_native.EOM_STOP_AT_END if stop_at_end else 0) | (_native.MODES_TENSOR if tensor else 0)
            target = np.full(run.size, np.nan) if N_eval is None else N_eval - lane_start[run]
            kappa = h[found] * math.exp(N_sub)
            lane_p = p if p.ndim == 1 else np.ascontiguousarray(rows[found])
            got, ends, st = lib.mode_spectra(lane_p, np.ascontiguousarray(start[found]), np.ascontiguousarray(kappa), target, max_steps, _METHODS[solver], max_err,
                                             dt or 0.0, flags)  # fmt: skip
            _mode_stage2_result(out, n_end, status, run, N_eval, got, ends, st)
    return out, h_exit.reshape(B, K), n_exit, lane_start, n_end, status


def _spectra_at_k(artifact, tensor, pars, ln_k, fields_init, derivatives_init, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    p, pts, x, v, off, N_eval, N_sub, max_steps, max_err, dt = _check_at_k(artifact, pars, ln_k, fields_init, derivatives_init, offset, N_eval, N_sub, max_steps,
                                                                           max_err, solver, dt, stop_at_end)  # fmt: skip
    out, h_exit, n_exit, lane_start, n_end, status = _mode_lanes_at_k(artifact, tensor, p, pts, x, v, off, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)
    B, K = h_exit.shape
    shift = lane_start.reshape(B, K)
    with np.errstate(invalid="ignore"):
        k = h_exit * np.exp(n_exit)
    status = status.reshape(B, K)
    if tensor:
        out = out.reshape(8, B, K)
        res = TensorSpectra(out[0], k, out[5] + shift, out[7], out[1] + 1j * out[2], n_end.reshape(B, K) + shift, status)
    else:
        out = out.reshape(22, B, K)
        q = out[3:11].reshape(2, 2, 2, B, K)  # [I][J][re, im]
        modes = np.moveaxis(q[:, :, 0] + 1j * q[:, :, 1], (0, 1), (2, 3))
        res = PowerSpectra(out[0], out[1], out[2], k, out[19] + shift, out[21], modes, n_end.reshape(B, K) + shift, status)
    return res, ExitPoints(pts, n_exit)


def power_spectra_at_k(artifact: CompilationArtifact, pars, ln_k, fields_init, derivatives_init, *, offset=None, N_eval=None, N_sub: float = 5.0,
                       max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True):  # fmt: skip
    """``power_spectra`` on a grid of comoving wavenumbers that all trajectories share: ``(spectra, exits)`` with ``spectra`` the
    :class:`PowerSpectra` of (B, K) arrays and ``exits`` the :class:`ExitPoints` -- the requested ``ln_k`` and the located ``N_exit``
    (B, K).  Row b is DEFINED as ``power_spectra`` of trajectory b alone with ``N_exit`` = the e-fold counts at which its own ln(a H)
    crosses ``offset[b] + ln_k`` -- bit for bit, in every member; ``k`` is as computed, H_exit e^N_exit, and equals
    e^(offset + ln_k) up to the crossing's residual.

    ``horizon_crossings`` runs first (``ln_k``, ``offset`` and the units as documented there).  Then every mode's start state at
    N_exit - ``N_sub`` and its H at N_exit are taken from ``state_at_efolds`` lanes with per-lane targets, which is what
    ``solve_eom_sampled`` gives ``power_spectra``'s stage 1; then ``power_spectra``'s stage 2 runs unchanged.  A lane whose mode was
    outside the horizon at the start, or has N_exit < ``N_sub``, gets the status ``OUTSIDE_AT_START`` (a code of this module; no kernel
    returns it) and NaN values; a crossing the trajectory never reached keeps ``horizon_crossings``' status.  ``N_eval``: None, or an
    e-fold count since the start, which must be > ``N_sub`` (checked before the device is touched) and above every located N_exit
    (checked once they are known).  Every other argument is ``power_spectra``'s."""
    return _spectra_at_k(artifact, False, pars, ln_k, fields_init, derivatives_init, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)


def tensor_spectra_at_k(artifact: CompilationArtifact, pars, ln_k, fields_init, derivatives_init, *, offset=None, N_eval=None, N_sub: float = 5.0,
                        max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None, stop_at_end: bool = True):  # fmt: skip
    """``tensor_spectra`` on a grid of comoving wavenumbers that all trajectories share: ``power_spectra_at_k``'s tensor twin, with the
    same arguments, checks, crossings and ``(spectra, exits)`` -- ``spectra`` a :class:`TensorSpectra`, ``k`` and ``exits``
    ``power_spectra_at_k``'s bit for bit."""
    return _spectra_at_k(artifact, True, pars, ln_k, fields_init, derivatives_init, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)


def _check_dlnk(dlnk):
    try:
        dlnk = float(dlnk)
    except (TypeError, ValueError):
        raise ValueError("dlnk must be a number") from None
    if not (math.isfinite(dlnk) and dlnk > 0.0):
        raise ValueError(f"dlnk must be finite and > 0 (got {dlnk})")
    return dlnk


def _observables_at_k(artifact, pars, ln_k, fields_init, derivatives_init, dlnk, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end):
    """``observables_at_k`` and the pivots' located N_exit (B, K)"""
    dlnk = _check_dlnk(dlnk)
    pivots = _check_ln_k(ln_k)
    pts, inverse = np.unique(np.concatenate([pivots - dlnk, pivots, pivots + dlnk]), return_inverse=True)
    kw = dict(offset=offset, N_eval=N_eval, N_sub=N_sub, max_steps=max_steps, max_err=max_err, solver=solver, dt=dt, stop_at_end=stop_at_end)
    scalar, exits = power_spectra_at_k(artifact, pars, pts, fields_init, derivatives_init, **kw)
    tensor, _ = tensor_spectra_at_k(artifact, pars, pts, fields_init, derivatives_init, **kw)
    cols = inverse.reshape(3, pivots.size)
    return observables_from_spectra(scalar, tensor, cols, ENDED if N_eval is None else TARGET), exits.N_exit[:, cols[1]]


def observables_at_k(artifact: CompilationArtifact, pars, ln_k, fields_init, derivatives_init, *, dlnk: float = 0.5, offset=None, N_eval=None,
                     N_sub: float = 5.0, max_steps: int = 1_000_000, max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None,
                     stop_at_end: bool = True) -> Observables:  # fmt: skip
    """``observables`` at K pivot wavenumbers ``ln_k`` that all trajectories share: ``power_spectra_at_k`` and ``tensor_spectra_at_k``
    on the sorted, de-duplicated union of ``ln_k - dlnk``, ``ln_k`` and ``ln_k + dlnk``, then ``observables_from_spectra``.  The
    stencil is uniform in ln k up to the crossings' residual (``log_slopes`` still takes every trajectory's ``k`` as computed), and
    the derivative is taken at fixed comoving k, not at a fixed e-fold count: n_s, alpha_s and n_t of two trajectories refer to the
    same scales.  ``dlnk`` must be finite and > 0; the other arguments are ``power_spectra_at_k``'s.  A pivot any of whose six lanes was
    outside the horizon at the start has the status ``OUTSIDE_AT_START`` and NaN values."""
    return _observables_at_k(artifact, pars, ln_k, fields_init, derivatives_init, dlnk, offset, N_eval, N_sub, max_steps, max_err, solver, dt, stop_at_end)[0]


def reheating_offset(k_mpc: float = 0.05, *, w_reh: float = 1.0 / 3.0, N_reh: float = 0.0, g_reh: float = 106.75, gs_reh: float = 106.75) -> float:
    """The constant A of the pivot matching: a mode of physical wavenumber ``k_mpc`` (in 1 / Mpc) today left the horizon where

        ln(a H) = N_end + ln(H_end) / 2 + A,
        A = ln(k / T_0) + ln(3) / 4 + ln(30 / (pi^2 g_reh)) / 4 + ln(gs_reh / gs_0) / 3 + (1 - 3 w_reh) N_reh / 4

    in the solver's units (3 H^2 = rho, reduced Planck mass 1, a = 1 at the trajectory's start): entropy is conserved after
    reheating, rho_end = 3 H_end^2, and reheating lasts ``N_reh`` e-folds with the equation of state ``w_reh`` before the plasma of
    ``g_reh`` energy and ``gs_reh`` entropy degrees of freedom is thermal.  T_0 = 2.7255 K, gs_0 = 43 / 11, 1 / Mpc = 6.39493e-39 GeV
    and 1 K = 8.617333e-14 GeV; the Planck mass cancels in k / T_0 and enters through H only.  The defaults -- 0.05 / Mpc, 106.75
    degrees of freedom, instant reheating -- give A = -61.37.  A pure function: ``k_mpc``, ``g_reh`` and ``gs_reh`` must be finite
    and > 0, ``N_reh`` finite and >= 0, -1/3 < ``w_reh`` <= 1."""
    try:
        k_mpc, w_reh, N_reh, g_reh, gs_reh = float(k_mpc), float(w_reh), float(N_reh), float(g_reh), float(gs_reh)
    except (TypeError, ValueError):
        raise ValueError("reheating_offset takes numbers") from None
    for name, value in (("k_mpc", k_mpc), ("g_reh", g_reh), ("gs_reh", gs_reh)):
        if not (math.isfinite(value) and value > 0.0):
            raise ValueError(f"{name} must be finite and > 0 (got {value})")
    if not (math.isfinite(N_reh) and N_reh >= 0.0):
        raise ValueError(f"N_reh must be finite and >= 0 (got {N_reh})")
    if not (-1.0 / 3.0 < w_reh <= 1.0):
        raise ValueError(f"w_reh must be in (-1/3, 1] (got {w_reh})")
    return (math.log(k_mpc * MPC_INV_GEV / (T_CMB_K * KELVIN_GEV)) + 0.25 * math.log(3.0) + 0.25 * math.log(30.0 / (math.pi**2 * g_reh))
            + math.log(gs_reh / GS_TODAY) / 3.0 + 0.25 * (1.0 - 3.0 * w_reh) * N_reh)  # fmt: skip


def _check_pivot_grid(artifact, pars, start_stop, N0, N1, A, derivatives_init, max_steps, max_err, solver):
    """The argument checks of the pivot maps: (p, init (N0 N1, 4), A (N0 N1,), N0, N1, max_steps, max_err)."""
    max_steps, _, max_err, _ = _check_common(artifact, max_steps, max_err, solver, None)
    ss, N0, N1, d = _check_grid(start_stop, N0, N1, derivatives_init)
    try:
        a = np.asarray(A, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("A must be a number or an (N0, N1) array of numbers") from None
    if a.ndim != 0 and a.shape != (N0, N1):
        raise InflatoxShapeError(f"A must be a scalar or have shape ({N0}, {N1}) (got {a.shape})")
    if not np.isfinite(a).all():
        raise ValueError("A must be finite")
    p = _parameter_row(artifact, pars, "the pivot maps take")
    init = _grid_init(ss, N0, N1, d)
    return p, init, np.broadcast_to(a, (N0, N1)).reshape(-1), N0, N1, max_steps, max_err


def _pivot_crossing(artifact, p, init, A, ln_k, max_steps, max_err, solver):
    """``inflation_end`` on the points ``init`` and, on those that ended, the crossing of ln(a H) = N_end + ln(H_end) / 2 + A + ln_k:
    (end, pivot L (n,), state (n, 5), N (n,), status (n,)) -- NaN where nothing was found."""
    n = init.shape[0]
    end = inflation_end(artifact, p, init[:, :2], init[:, 2:], max_steps=max_steps, max_err=max_err, solver=solver)
    status = end.status.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        pivot = end.N_end + 0.5 * np.log(end.state[:, 4]) + A
    state, n_at = np.full((n, 5), np.nan), np.full(n, np.nan)
    run = np.flatnonzero((end.status == ENDED) & np.isfinite(pivot))
    if run.size:
        cr = horizon_crossings(artifact, p, [ln_k], init[run, :2], init[run, 2:], offset=pivot[run], max_steps=max_steps, max_err=max_err, solver=solver)
        state[run], n_at[run] = cr.states[:, 0], cr.N[:, 0]
        status[run] = np.where(cr.n_before == 1, ENDED_SHORT, cr.status)
    return end, pivot, state, n_at, status


def pivot_exit_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, A, derivatives_init=(0.0, 0.0), max_steps: int = 100_000,
                   max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """The state at which a physical pivot scale leaves the horizon, from every point of the (N0, N1) grid of ``efolds_map`` (same
    arguments): ``(state, N_star, N_end)`` with ``state`` (N0, N1, 5) = phi^0, phi^1, chi^0, chi^1, H where

        ln(a H) = N_end + ln(H_end) / 2 + A,

    ``N_star`` (N0, N1) = N_end - N there -- it follows from the trajectory, N_star = ln H_star - ln(H_end) / 2 - A, and differs from
    point to point -- and ``N_end`` (N0, N1).  ``A`` (a number, or (N0, N1)) holds the wavenumber and the reheating history:
    ``reheating_offset``.  Two passes of O(N0 * N1) memory: ``inflation_end`` on the grid, then ``horizon_crossings`` with that offset
    and ``ln_k = [0]`` on the points that ended.  NaN where nothing was found; ``return_status=True`` adds the (N0, N1) int8 status
    map: ``TARGET`` where the state was found, ``ENDED_SHORT`` where the pivot was outside the horizon at the start -- inflation from
    this point is too short for it --, ``ENDED`` where inflation ended before the pivot left (A too large), and ``inflation_end``'s
    status where inflation did not end."""
    p, init, a, N0, N1, max_steps, max_err = _check_pivot_grid(artifact, pars, start_stop, N0, N1, A, derivatives_init, max_steps, max_err, solver)
    end, _, state, n_at, status = _pivot_crossing(artifact, p, init, a, 0.0, max_steps, max_err, solver)
    out = (state.reshape(N0, N1, 5), (end.N_end - n_at).reshape(N0, N1), end.N_end.reshape(N0, N1))
    return (*out, status.reshape(N0, N1)) if return_status else out


def pivot_observables_map(artifact: CompilationArtifact, pars, start_stop, N0: int, N1: int, A, dlnk: float = 0.5, N_sub: float = 5.0,
                          derivatives_init=(0.0, 0.0), max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", *, return_status: bool = False):  # fmt: skip
    """n_s, r and the other :class:`Observables` at a physical pivot scale as (N0, N1) maps: ``(obs, state, N_star, N_end)``.  As in
    ``pivot_exit_map`` the pivot leaves the horizon where ln(a H) = L_star = N_end + ln(H_end) / 2 + A.  ``state`` (N0, N1, 5) is the
    crossing of L_star - (``dlnk`` + ``N_sub``): since d ln(a H) / dN = 1 - epsilon_H < 1, it lies at least ``N_sub`` e-folds before the
    exit of the lowest of the three modes.  From it (H taken again from the Friedmann constraint, as in ``observables_map``)
    ``observables_at_k`` runs with ``ln_k = [0]`` and ``offset`` = L_star minus the restart's N -- a = 1 at the restart -- to the end of
    inflation.  ``N_star`` (N0, N1) = N_end minus the pivot's own exit, and ``N_end`` (N0, N1) is ``inflation_end``'s.  NaN where nothing
    was found; ``obs.status`` and, with ``return_status=True``, a fifth member are the (N0, N1) status map: ``pivot_exit_map``'s for the
    restart state, with ``observables_at_k``'s status (``ENDED`` where the values are valid) in place of ``TARGET``."""
    N_sub = _check_n_sub(N_sub)
    dlnk = _check_dlnk(dlnk)
    p, init, a, N0, N1, max_steps, max_err = _check_pivot_grid(artifact, pars, start_stop, N0, N1, A, derivatives_init, max_steps, max_err, solver)
    end, pivot, state, n_at, status = _pivot_crossing(artifact, p, init, a, -(dlnk + N_sub), max_steps, max_err, solver)

    def to_the_end(x, v, run):
        obs, n_exit = _observables_at_k(artifact, p, [0.0], x, v, dlnk, pivot[run] - n_at[run], None, N_sub, max_steps, max_err, solver, None, True)
        return [member[:, 0] for member in obs[:-1]] + [end.N_end[run] - (n_at[run] + n_exit[:, 0])], obs.status[:, 0]

    # every point whose restart state was located goes on, whatever its status
    (*values, n_star), status = _second_stage(state.reshape(N0, N1, 5), status.reshape(N0, N1), np.int8, [()] * len(Observables._fields), to_the_end,
                                              run=np.flatnonzero(np.isfinite(n_at)))  # fmt: skip
    out = (Observables(*values, status), state.reshape(N0, N1, 5), n_star, end.N_end.reshape(N0, N1))
    return (*out, status) if return_status else out
