"""Reheating on the GPU: a trajectory continued past the end of inflation, its fields decaying into a radiation bath at a constant
rate Gamma, until the bath dominates -- and from the state located there the length of reheating ``N_reh``, its mean equation of
state ``w_reh`` and the offset A of the pivot matching, which ``inflatox_amd.background.reheating_offset`` otherwise takes from
numbers the user types in.

In the units of ``inflatox_amd.background`` (reduced Planck mass 1, cosmic time, 3 H^2 = rho) a lane integrates
y = (phi^0, phi^1, chi^0, chi^1, H, N, rho_r):

    dphi^a/dt  = chi^a
    dchi^a/dt  = -eom^a(phi, chi) - (3 H + Gamma) chi^a
    dH/dt      = V - 3 H^2 + rho_r / 3
    dN/dt      = H
    drho_r/dt  = -4 H rho_r + Gamma G_ab chi^a chi^b

from H_0 = sqrt((V + G_ab chi^a chi^b / 2 + rho_r) / 3), N = 0, t = 0, with the steppers and the step control of ``solve_eom`` on seven
components (the error norm covers phi, chi, H and rho_r) and stops ``REHEATED`` at the first accepted step whose end state has
Omega_r = rho_r / (3 H^2) >= ``omega_r``; the state is located on that step's cubic Hermite dense output where
rho_r - 3 omega_r H^2 = 0 (csrc/inflx_reheating.h).  ``reheating`` runs B such lanes, ``reheating_map`` runs them from the located end
of inflation of every point of a grid, ``offset_from_reheating`` turns the result into A, and ``pivot_observables_map_reheated``
puts that A under ``background.pivot_observables_map``.

What is not modelled: Gamma is one constant per lane -- no per-field and no field-dependent rates --; every oscillation of the fields
is resolved by the stepper, so the cost grows with m / Gamma (no averaged treatment of Gamma << m); perturbations are not carried
through reheating, and spectra are still read at epsilon_H = 1.  The kernels live in ``<artefact>.reheating``
(``CompilationArtifact.ensure_reheating``), a companion object of its own.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import background
from ._native import InflatoxShapeError
from .background import _METHODS, _check_common, _check_fields, _check_grid, _companion_dylib, _grid_init, _parameter_row, _pars, _second_stage
from .compiler import CompilationArtifact

__all__ = ["reheating", "reheating_map", "offset_from_reheating", "pivot_observables_map_reheated", "Reheating", "REHEATED", "STATUS"]

#: ``status`` of a lane whose radiation reached ``omega_r`` (csrc/inflx_reheating.h ``INFLX_RH_REHEATED``)
REHEATED = 10
STATUS = {**background.STATUS, REHEATED: "rho_r / (3 H^2) reached omega_r; the state is the one located there (reheating)"}


class Reheating(NamedTuple):
    """What :func:`reheating` returns, for B lanes.  ``state`` (B, 5): phi^0, phi^1, chi^0, chi^1, H; ``rho_r`` (B,); ``N_reh`` and
    ``t_reh`` (B,): e-folds and cosmic time since the lane's start; ``H_start`` (B,): H_0 from the constraint; ``w_reh`` (B,): the mean
    equation of state -1 - (2/3) ln(H_reh / H_0) / N_reh, NaN at N_reh = 0; ``A_shift`` (B,) = N_reh + ln(H_reh / H_0) / 2 =
    (1 - 3 w_reh) N_reh / 4; ``omega_r`` (B,): rho_r / (3 H^2) at the returned state; ``status`` (B,) int8.  For a ``REHEATED`` lane all
    of it is read at the located state.  Every other lane returns the last state it held in ``state``, ``rho_r``, ``t_reh`` and
    ``omega_r``, and NaN in ``N_reh``, ``w_reh`` and ``A_shift``."""

    state: np.ndarray
    rho_r: np.ndarray
    N_reh: np.ndarray
    t_reh: np.ndarray
    H_start: np.ndarray
    w_reh: np.ndarray
    A_shift: np.ndarray
    omega_r: np.ndarray
    status: np.ndarray


def _reheating_dylib(artifact):
    return _companion_dylib(artifact, "reheating")


def _check_omega_r(omega_r):
    try:
        omega_r = float(omega_r)
    except (TypeError, ValueError):
        raise ValueError("omega_r must be a number") from None
    if not (0.0 < omega_r < 1.0):
        raise ValueError(f"omega_r must be in (0, 1) (got {omega_r})")
    return omega_r


def _check_rates(value, name, shape):
    """``value`` as a float64 array of ``shape``: a number or an array of that shape, finite and >= 0"""
    try:
        a = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or an array of numbers") from None
    if a.ndim != 0 and a.shape != shape:
        raise InflatoxShapeError(f"{name} must be a scalar or have shape {shape} (got {a.shape})")
    if not (np.isfinite(a).all() and (a >= 0.0).all()):
        raise ValueError(f"{name} must be finite and >= 0")
    return np.ascontiguousarray(np.broadcast_to(a, shape))


def _result(states, t, h_start, status) -> Reheating:
    hit = status == REHEATED
    hub, n, rho = states[:, 4], states[:, 5], states[:, 6]
    with np.errstate(invalid="ignore", divide="ignore"):
        ln_ratio = np.log(hub / h_start)
        w = np.where(hit & (n != 0.0), -1.0 - (2.0 / 3.0) * ln_ratio / n, np.nan)
        shift = np.where(hit, n + 0.5 * ln_ratio, np.nan)
        omega = rho / (3.0 * hub * hub)
    return Reheating(states[:, :5], rho, np.where(hit, n, np.nan), t, h_start, w, shift, omega, status)


def _run(artifact, p, init, gamma, rho, omega_r, max_steps, solver, max_err, dt) -> Reheating:
    return _result(*_reheating_dylib(artifact).reheating(p, init, gamma, rho, omega_r, max_steps, _METHODS[solver], max_err, dt or 0.0))


def reheating(artifact: CompilationArtifact, pars, Gamma, fields_init, derivatives_init, *, omega_r: float = 0.99, rho_r_init=0.0, max_steps: int = 100_000,
              max_err: float = 1e-8, solver: str = "rkf", dt: float | None = None) -> Reheating:  # fmt: skip
    """B trajectories from ``fields_init`` and ``derivatives_init`` (B, 2) whose fields decay into radiation at the rate ``Gamma`` (a
    number or (B,), finite and >= 0), each until the radiation's share of the energy reaches ``omega_r`` (0 < omega_r < 1).  ``pars`` is
    one parameter row or (B, P); ``rho_r_init`` (a number or (B,), finite and >= 0) is the radiation the lanes start with; the other
    arguments are ``inflation_end``'s.  The equations, the event and the members of the result are described in the module's docstring
    and in :class:`Reheating`.

    A lane stops ``REHEATED`` at the first accepted step whose end state has rho_r - 3 omega_r H^2 >= 0, and its state is the point of
    that step's dense output where this function vanishes: the Illinois iteration ``inflation_end`` uses, on a polynomial in theta, so
    no model is evaluated.  A lane that starts with Omega_r >= ``omega_r`` is ``REHEATED`` at its start, N_reh = 0 and w_reh NaN.
    ``COMPLETE`` where ``max_steps`` accepted steps ran out first -- Gamma = 0 without initial radiation never reheats, which is that
    and no error --, ``NONFINITE``, ``REJECTED`` and ``UNDERFLOW`` as in ``solve_eom``.  The cost grows with m / Gamma, since every
    oscillation of the fields is resolved; no averaged treatment of Gamma << m exists here.  The kernels are built into
    ``<artefact>.reheating`` on first use.  Bad arguments raise before anything runs on the device."""
    max_steps, _, max_err, dt = _check_common(artifact, max_steps, max_err, solver, dt)
    omega_r = _check_omega_r(omega_r)
    x, v = _check_fields(fields_init, derivatives_init)
    B = x.shape[0]
    gamma = _check_rates(Gamma, "Gamma", (B,))
    rho = _check_rates(rho_r_init, "rho_r_init", (B,))
    p = _pars(artifact, pars, B)
    return _run(artifact, p, np.concatenate([x, v], axis=1), gamma, rho, omega_r, max_steps, solver, max_err, dt)


def _check_map(artifact, pars, Gamma, start_stop, N0, N1, derivatives_init, omega_r, max_steps, max_err, solver):
    """The argument checks of the two maps: (p, init (N0 N1, 4), gamma (N0 N1,), omega_r, N0, N1, max_steps, max_err)."""
    max_steps, _, max_err, _ = _check_common(artifact, max_steps, max_err, solver, None)
    omega_r = _check_omega_r(omega_r)
    ss, N0, N1, d = _check_grid(start_stop, N0, N1, derivatives_init)
    gamma = _check_rates(Gamma, "Gamma", (N0, N1)).reshape(-1)
    p = _parameter_row(artifact, pars, "the reheating maps take")
    return p, _grid_init(ss, N0, N1, d), gamma, omega_r, N0, N1, max_steps, max_err


def _map(artifact, p, init, gamma, omega_r, N0, N1, max_steps, max_err, solver):
    end = background.inflation_end(artifact, p, init[:, :2], init[:, 2:], max_steps=max_steps, max_err=max_err, solver=solver)

    def decay(x, v, run):
        reh = _run(artifact, p, np.concatenate([x, v], axis=1), gamma[run], np.zeros(run.size), omega_r, max_steps, solver, max_err, None)
        return list(reh[:-1]), reh.status

    planes = [(5,)] + [()] * (len(Reheating._fields) - 2)
    values, status = _second_stage(end.state.reshape(N0, N1, 5), end.status.reshape(N0, N1), np.int8, planes, decay, run=np.flatnonzero(end.status == background.ENDED))
    return Reheating(*values, status), end.N_end.reshape(N0, N1), status


def reheating_map(artifact: CompilationArtifact, pars, Gamma, start_stop, N0: int, N1: int, *, derivatives_init=(0.0, 0.0), omega_r: float = 0.99,
                  max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf"):  # fmt: skip
    """Reheating after inflation from every point of the (N0, N1) grid of ``efolds_map`` (same grid arguments, one parameter row):
    ``inflation_end`` on the grid, then ``reheating`` from the located end states of the points that ``ENDED`` -- fields and
    velocities; H is taken again from the constraint, as in the other two-stage maps, and the radiation starts at 0 --, so that
    ``N_reh`` counts from the end of inflation.  ``Gamma`` is a number or (N0, N1).  Returns ``(reh, N_end, status)``: ``reh`` a
    :class:`Reheating` of (N0, N1) members (``state`` (N0, N1, 5)), NaN where inflation did not end; ``N_end`` (N0, N1) is
    ``inflation_end``'s; ``status`` (N0, N1) int8 is ``reheating``'s where inflation ended and ``inflation_end``'s elsewhere."""
    p, init, gamma, omega_r, N0, N1, max_steps, max_err = _check_map(artifact, pars, Gamma, start_stop, N0, N1, derivatives_init, omega_r, max_steps, max_err, solver)
    return _map(artifact, p, init, gamma, omega_r, N0, N1, max_steps, max_err, solver)


def offset_from_reheating(reh: Reheating, k_mpc: float = 0.05, *, g_reh: float = 106.75, gs_reh: float = 106.75):
    """The constant A of the pivot matching (``background.reheating_offset``) with the reheating history of ``reh`` in place of a
    guessed ``w_reh`` and ``N_reh``: the instant-reheating value ``reheating_offset(k_mpc, g_reh=, gs_reh=)`` plus ``reh.A_shift`` =
    (1 - 3 w_reh) N_reh / 4.  It does not pass through ``reheating_offset(w_reh=...)``, whose range (-1/3, 1] would refuse lanes with a
    second accelerated phase after the first end of inflation.  NaN where the lane is not ``REHEATED``.  A pure function."""
    instant = background.reheating_offset(k_mpc, g_reh=g_reh, gs_reh=gs_reh)
    return np.where(np.asarray(reh.status) == REHEATED, instant + np.asarray(reh.A_shift, dtype=np.float64), np.nan)


def pivot_observables_map_reheated(artifact: CompilationArtifact, pars, Gamma, start_stop, N0: int, N1: int, k_mpc: float = 0.05, *, g_reh: float = 106.75,
                                   gs_reh: float = 106.75, omega_r: float = 0.99, dlnk: float = 0.5, N_sub: float = 5.0, derivatives_init=(0.0, 0.0),
                                   max_steps: int = 100_000, max_err: float = 1e-8, solver: str = "rkf", return_status: bool = False):  # fmt: skip
    """``background.pivot_observables_map`` with the offset A of every grid point computed from its own reheating: ``reheating_map``
    with the decay rate ``Gamma`` (a number or (N0, N1)), A = ``offset_from_reheating`` of it for the wavenumber ``k_mpc`` (in 1 / Mpc)
    and the degrees of freedom ``g_reh``, ``gs_reh``, then ``pivot_observables_map`` with that A.  A point that did not reheat is
    handed the instant-reheating value, so that the array is finite, and is NaN in every member afterwards, with its reheating status.
    Returns ``(obs, state, N_star, N_end, reh)`` -- the first four as ``pivot_observables_map`` returns them, ``reh`` the
    :class:`Reheating` map -- and with ``return_status=True`` the (N0, N1) int8 status map as a sixth member.  ``inflation_end`` runs
    on the grid twice, once in each half.  Perturbations are not carried through reheating: the spectra are read at epsilon_H = 1."""
    instant = background.reheating_offset(k_mpc, g_reh=g_reh, gs_reh=gs_reh)
    N_sub = background._check_n_sub(N_sub)
    dlnk = background._check_dlnk(dlnk)
    p, init, gamma, omega_r, N0, N1, max_steps, max_err = _check_map(artifact, pars, Gamma, start_stop, N0, N1, derivatives_init, omega_r, max_steps, max_err, solver)
    reh, _, reh_status = _map(artifact, p, init, gamma, omega_r, N0, N1, max_steps, max_err, solver)
    hit = reh_status == REHEATED
    A = np.where(hit, instant + reh.A_shift, instant)
    obs, state, n_star, n_end, status = background.pivot_observables_map(artifact, p, start_stop, N0, N1, A, dlnk, N_sub, derivatives_init, max_steps, max_err, solver,
                                                                         return_status=True)  # fmt: skip
    status = np.where(hit, status, reh_status).astype(np.int8)
    values = [np.where(hit, member, np.nan) for member in obs[:-1]]
    out = (background.Observables(*values, status), np.where(hit[..., None], state, np.nan), np.where(hit, n_star, np.nan), n_end, reh)
    return (*out, status) if return_status else out
