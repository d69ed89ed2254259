"""The argument checks of ``inflatox_amd.background``, one literal table: every public function that checks its arguments, every
distinct check of the blocks the functions share (the common options, fields and velocities, the sample lists, the grid, the
parameter row, N_star), and for every function a call with two faults, where the message of the earlier check must win.  The calls
run on a stub artefact with the device out of reach, so a check that passes a bad argument on fails the test as well.  The messages
are those the functions raised when the table was written, exception type and text, and the order of the checks is part of it."""

import math
import types

import numpy as np
import pytest

from inflatox_amd import background as bg
from inflatox_amd._native import InflatoxShapeError
from inflatox_amd.compiler import CompilationArtifact

A = types.SimpleNamespace(n_fields=2, n_parameters=3)
A3 = types.SimpleNamespace(n_fields=3, n_parameters=3)
P = [1.0, 2.0, 3.0]
X = [[1.0, 2.0], [3.0, 4.0]]
V = [[0.0, 0.0], [0.0, 0.0]]
SS = [[0.0, 1.0], [2.0, 3.0]]
P13, P33, P63 = np.ones((1, 3)), np.ones((3, 3)), np.ones((6, 3))
SP = types.SimpleNamespace(P_R=np.ones((2, 4)), P_S=np.ones((2, 4)), C_RS=np.ones((2, 4)))

# fmt: off
CASES = [
    # ---- the common checks (_check_common), every one through solve_eom_batch
    (lambda: bg.solve_eom_batch(A3, P, 10, X, V), InflatoxShapeError, "the background solver requires a 2-field model (model has 3 fields)"),
    (lambda: bg.solve_eom_batch(A, P, 1.5, X, V), ValueError, "steps and substeps must be integers"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, substeps=2.0), ValueError, "steps and substeps must be integers"),
    (lambda: bg.solve_eom_batch(A, P, 0, X, V), ValueError, "steps must be at least 1 (got 0)"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, substeps=0), ValueError, "substeps must be in [1, 2^32) (got 0)"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, substeps=2**32), ValueError, "substeps must be in [1, 2^32) (got 4294967296)"),
    (lambda: bg.solve_eom_batch(A, P, 2**40, X, V, substeps=2**31), ValueError, "steps x substeps exceeds 2^62 accepted steps"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, 0.0), ValueError, "max_err must be a positive finite number (got 0.0)"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, math.inf), ValueError, "max_err must be a positive finite number (got inf)"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, 1e-6, "euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, dt=-1.0), ValueError, "dt must be None (adaptive) or a positive finite step (got -1.0)"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, dt=math.nan), ValueError, "dt must be None (adaptive) or a positive finite step (got nan)"),
    (lambda: bg.solve_eom_batch(A, P, 0, X, V, 0.0, "euler"), ValueError, "steps must be at least 1 (got 0)"),  # two faults: steps before max_err before solver
    (lambda: bg.solve_eom_batch(A, P, 10, X, V, 1e-6, "euler", dt=-1.0), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before dt
    # ---- fields and velocities (B, 2), parameter rows
    (lambda: bg.solve_eom_batch(A, P, 10, [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.solve_eom_batch(A, P, 10, [[1.0, 2.0, 3.0]], [[0.0, 0.0, 0.0]]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (1, 3) and (1, 3))"),
    (lambda: bg.solve_eom_batch(A, P, 10, X, [[0.0, 0.0]]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2, 2) and (1, 2))"),
    (lambda: bg.solve_eom_batch(A, [1.0, 2.0], 10, X, V), InflatoxShapeError, "model has 3 parameters (got 2)"),
    (lambda: bg.solve_eom_batch(A, P33, 10, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.solve_eom_batch(A, np.ones((2, 2, 3)), 10, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (2, 2, 3))"),
    (lambda: bg.solve_eom_batch(A, P, 10, [1.0, 2.0], V, 1e-6, "euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before fields
    (lambda: bg.solve_eom_batch(A, P33, 10, [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before pars
    (lambda: bg.solve_eom_batch_device(A, P, 10, [1.0, 2.0], V, 1e-6, "euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before fields
    (lambda: bg.solve_eom_batch_device(A, P33, 10, [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before pars
    (lambda: bg.solve_eom_batch_device(A, P33, 10, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.solve_eom(A, P13, 10, [1.0, 2.0], [0.0, 0.0]), InflatoxShapeError, "pars must be one parameter row (got shape (1, 3))"),
    (lambda: bg.solve_eom(A, P, 10, [1.0, 2.0, 3.0], [0.0, 0.0, 0.0]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (1, 3) and (1, 3))"),
    (lambda: bg.solve_eom(A, P13, 0, [1.0, 2.0], [0.0, 0.0]), InflatoxShapeError, "pars must be one parameter row (got shape (1, 3))"),  # two faults: the parameter row before steps
    # ---- the grid: start_stop, N0, N1, derivatives_init, one parameter row
    (lambda: bg.efolds_map(A, P, [0.0, 1.0], 3, 2), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),
    (lambda: bg.efolds_map(A, P, SS, 0, 2), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.efolds_map(A, P, SS, 3, -1), ValueError, "the grid needs at least one point per axis (got 3 x -1)"),
    (lambda: bg.efolds_map(A, P, SS, 1.5, 2), TypeError, "'float' object cannot be interpreted as an integer"),
    (lambda: bg.efolds_map(A, P, SS, 3, 2, (0.0, 0.0, 0.0)), InflatoxShapeError, "derivatives_init must hold two velocities (got 3)"),
    (lambda: bg.efolds_map(A, [1.0, 2.0], SS, 3, 2), InflatoxShapeError, "model has 3 parameters (got 2)"),
    (lambda: bg.efolds_map(A, P63, SS, 3, 2), InflatoxShapeError, "pars must have shape (3,) or (1, 3) (got (6, 3))"),
    (lambda: bg.efolds_map(A, P13, SS, 3, 2), InflatoxShapeError, "efolds_map takes one parameter row"),
    (lambda: bg.efolds_map(A, P, [0.0, 1.0], 0, 2, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before start_stop
    (lambda: bg.efolds_map(A, P, [0.0, 1.0], 0, 2), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),  # two faults: start_stop before N0
    (lambda: bg.efolds_map(A, P, SS, 0, 2, (0.0, 0.0, 0.0)), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),  # two faults: the grid before derivatives_init
    (lambda: bg.efolds_map(A, P13, SS, 3, 2, (0.0, 0.0, 0.0)), InflatoxShapeError, "derivatives_init must hold two velocities (got 3)"),  # two faults: derivatives_init before the parameter row
    (lambda: bg.efolds_map(A, P, SS, 3, 2, max_steps=0), ValueError, "steps must be at least 1 (got 0)"),
    # ---- state_at_efolds
    (lambda: bg.state_at_efolds(A, P, [1.0, 2.0], V, 10.0), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.state_at_efolds(A, P, X, V, [1.0, 2.0, 3.0]), InflatoxShapeError, "N_target must be a scalar or have shape (2,) (got (3,))"),
    (lambda: bg.state_at_efolds(A, P, X, V, math.nan), ValueError, "N_target must be finite"),
    (lambda: bg.state_at_efolds(A, P, X, V, [1.0, math.inf]), ValueError, "N_target must be finite"),
    (lambda: bg.state_at_efolds(A, P33, X, V, 10.0), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.state_at_efolds(A, P, [1.0, 2.0], V, math.nan, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before fields
    (lambda: bg.state_at_efolds(A, P, [1.0, 2.0], V, math.nan), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before N_target
    (lambda: bg.state_at_efolds(A, P33, X, V, math.nan), ValueError, "N_target must be finite"),  # two faults: N_target before pars
    # ---- the sample list of solve_eom_sampled and transfer_functions
    (lambda: bg.solve_eom_sampled(A, P, [1.0], X, V, at="x"), ValueError, "unknown sampling variable 'x': choose 'N' or 't'"),
    (lambda: bg.solve_eom_sampled(A, P, "abc", X, V), ValueError, "samples must be convertible to a float64 array"),
    (lambda: bg.solve_eom_sampled(A, P, [[1.0, 2.0]], X, V), InflatoxShapeError, "samples must be one-dimensional (got shape (1, 2))"),
    (lambda: bg.solve_eom_sampled(A, P, [], X, V), ValueError, "the number of samples must be in [1, 2^32) (got 0)"),
    (lambda: bg.solve_eom_sampled(A, P, [-1.0, 2.0], X, V), ValueError, "samples must be finite and >= 0"),
    (lambda: bg.solve_eom_sampled(A, P, [1.0, math.nan], X, V), ValueError, "samples must be finite and >= 0"),
    (lambda: bg.solve_eom_sampled(A, P, [1.0, 1.0], X, V), ValueError, "samples must be strictly increasing"),
    (lambda: bg.solve_eom_sampled(A, P, [2.0, 1.0], X, V), ValueError, "samples must be strictly increasing"),
    (lambda: bg.solve_eom_sampled(A, P, [1.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.solve_eom_sampled(A, P33, [1.0], X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.solve_eom_sampled(A, P, [], X, V, at="x", solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before at
    (lambda: bg.solve_eom_sampled(A, P, [], X, V, at="x"), ValueError, "unknown sampling variable 'x': choose 'N' or 't'"),  # two faults: at before samples
    (lambda: bg.solve_eom_sampled(A, P, [[1.0, 2.0]], [1.0, 2.0], V), InflatoxShapeError, "samples must be one-dimensional (got shape (1, 2))"),  # two faults: samples before fields
    (lambda: bg.solve_eom_sampled(A, P, [-1.0, -2.0], X, V), ValueError, "samples must be finite and >= 0"),  # two faults: the sign before the order
    (lambda: bg.solve_eom_sampled(A, P33, [1.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before pars
    (lambda: bg.transfer_functions(A, P, "abc", X, V), ValueError, "samples must be convertible to a float64 array"),
    (lambda: bg.transfer_functions(A, P, [[1.0, 2.0]], X, V), InflatoxShapeError, "samples must be one-dimensional (got shape (1, 2))"),
    (lambda: bg.transfer_functions(A, P, [], X, V), ValueError, "the number of samples must be in [1, 2^32) (got 0)"),
    (lambda: bg.transfer_functions(A, P, [-1.0], X, V), ValueError, "samples must be finite and >= 0"),
    (lambda: bg.transfer_functions(A, P, [2.0, 1.0], X, V), ValueError, "samples must be strictly increasing"),
    (lambda: bg.transfer_functions(A, P, [0.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.transfer_functions(A, P33, [0.0], X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.transfer_functions(A, P, [0.0], X, V, dq_dN="x"), ValueError, "dq_dN must be None, a number or a float64 array"),
    (lambda: bg.transfer_functions(A, P, [0.0], X, V, dq_dN=[1.0, 2.0, 3.0]), InflatoxShapeError, "dq_dN must be a scalar or have shape (2,) (got (3,))"),
    (lambda: bg.transfer_functions(A, P, [0.0], X, V, dq_dN=math.inf), ValueError, "dq_dN must be finite"),
    (lambda: bg.transfer_functions(A, P, [2.0, 1.0], [1.0, 2.0], V, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before samples
    (lambda: bg.transfer_functions(A, P, [2.0, 1.0], [1.0, 2.0], V), ValueError, "samples must be strictly increasing"),  # two faults: samples before fields
    (lambda: bg.transfer_functions(A, P33, [0.0], X, V, dq_dN="x"), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),  # two faults: pars before dq_dN
    # ---- N_star, and the maps built on horizon_exit_map
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, math.inf), ValueError, "N_star must be finite and >= 0 (got inf)"),
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, math.nan), ValueError, "N_star must be finite and >= 0 (got nan)"),
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, None), ValueError, "N_star must be a number"),  # as in the other maps; float()'s own error escaped here before
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, "x"), ValueError, "N_star must be a number"),  # as in the other maps; float()'s own error escaped here before
    (lambda: bg.horizon_exit_map(A, P, [0.0, 1.0], 3, 2, 55.0), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),
    (lambda: bg.horizon_exit_map(A, P, SS, 0, 2, 55.0), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.horizon_exit_map(A, P, SS, 3, 2, 55.0, (0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),
    (lambda: bg.horizon_exit_map(A, P13, SS, 3, 2, 55.0), InflatoxShapeError, "efolds_map takes one parameter row"),
    (lambda: bg.horizon_exit_map(A, P, [0.0, 1.0], 3, 2, -1.0, solver="euler"), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before solver
    (lambda: bg.horizon_exit_map(A, P, [0.0, 1.0], 3, 2, 55.0, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before start_stop
    (lambda: bg.turn_rate_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.turn_rate_map(A, P, SS, 3, 2, None), ValueError, "N_star must be a number"),  # as in the other maps; float()'s own error escaped here before
    (lambda: bg.turn_rate_map(A, P, [0.0, 1.0], 0, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    (lambda: bg.turn_rate_map(A, P, [0.0, 1.0], 0, 2), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),  # two faults: start_stop before N0
    (lambda: bg.mass_map(A, P, SS, 3, 2, math.nan), ValueError, "N_star must be finite and >= 0 (got nan)"),
    (lambda: bg.mass_map(A, P, SS, 3, 2, "x"), ValueError, "N_star must be a number"),  # as in the other maps; float()'s own error escaped here before
    (lambda: bg.mass_map(A, P, [0.0, 1.0], 0, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    (lambda: bg.mass_map(A, P13, SS, 3, 2, 55.0, (0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),  # two faults: derivatives_init before the parameter row
    (lambda: bg.transfer_map(A, P, SS, 1.5, 2, dq_dN=1.0), ValueError, "N0 and N1 must be integers"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, dq_dN=np.ones((2, 2))), InflatoxShapeError, "dq_dN must be a scalar or have shape (3, 2) (got (2, 2))"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, dq_dN="x"), ValueError, "dq_dN must be None, a number or a float64 array"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, dq_dN=[1.0, 2.0]), InflatoxShapeError, "dq_dN must be a scalar or have shape (1,) (got (2,))"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, dq_dN=math.nan), ValueError, "dq_dN must be finite"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, dq_dN=np.full((3, 2), math.inf)), ValueError, "dq_dN must be finite"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, None), ValueError, "N_star must be a number"),  # as in the other maps; float()'s own error escaped here before
    (lambda: bg.transfer_map(A, P, SS, 0, 2), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.transfer_map(A, P, SS, 3, 2, -1.0, dq_dN=math.nan), ValueError, "dq_dN must be finite"),  # two faults: dq_dN before N_star
    (lambda: bg.transfer_map(A, P, [0.0, 1.0], 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    # ---- kinematics and masses
    (lambda: bg.kinematics(A3, P, np.ones((2, 5))), InflatoxShapeError, "the kinematics require a 2-field model (model has 3 fields)"),
    (lambda: bg.masses(A3, P, np.ones((2, 5))), InflatoxShapeError, "the masses require a 2-field model (model has 3 fields)"),
    (lambda: bg.kinematics(A, P, "abc"), ValueError, "states must be convertible to a float64 array"),
    (lambda: bg.kinematics(A, P, np.ones(4)), InflatoxShapeError, "states must have shape (5,), (n, 5) or (B, S, 5) (got (4,))"),
    (lambda: bg.kinematics(A, P, np.ones((2, 2, 2, 5))), InflatoxShapeError, "states must have shape (5,), (n, 5) or (B, S, 5) (got (2, 2, 2, 5))"),
    (lambda: bg.kinematics(A, P33, np.ones((2, 5))), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.kinematics(A, P33, np.ones((2, 4, 5))), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.kinematics(A, [1.0], np.ones(5)), InflatoxShapeError, "model has 3 parameters (got 1)"),
    (lambda: bg.masses(A, P, np.ones((2, 6))), InflatoxShapeError, "states must have shape (5,), (n, 5) or (B, S, 5) (got (2, 6))"),
    (lambda: bg.masses(A, P33, np.ones((2, 5))), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.kinematics(A, P33, np.ones((2, 4))), InflatoxShapeError, "states must have shape (5,), (n, 5) or (B, S, 5) (got (2, 4))"),  # two faults: the states before pars
    (lambda: bg.masses(A, P33, np.ones((2, 4))), InflatoxShapeError, "states must have shape (5,), (n, 5) or (B, S, 5) (got (2, 4))"),  # two faults: the states before pars
    # ---- mode functions: power_spectra, tensor_spectra, spectrum_map
    (lambda: bg.power_spectra(A, P, "abc", X, V), ValueError, "N_exit must be convertible to a float64 array"),
    (lambda: bg.power_spectra(A, P, [[6.0]], X, V), InflatoxShapeError, "N_exit must be one-dimensional (got shape (1, 1))"),
    (lambda: bg.power_spectra(A, P, [], X, V), ValueError, "N_exit must hold at least one e-fold count"),
    (lambda: bg.power_spectra(A, P, [6.0], X, V, N_sub="x"), ValueError, "N_sub must be a number"),
    (lambda: bg.power_spectra(A, P, [6.0], X, V, N_sub=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: bg.power_spectra(A, P, [6.0], X, V, N_sub=math.inf), ValueError, "N_sub must be finite and > 0 (got inf)"),
    (lambda: bg.power_spectra(A, P, [4.0, 6.0], X, V), ValueError, "N_exit must be finite and >= N_sub = 5.0"),
    (lambda: bg.power_spectra(A, P, [6.0, math.nan], X, V), ValueError, "N_exit must be finite and >= N_sub = 5.0"),
    (lambda: bg.power_spectra(A, P, [6.0], X, V, stop_at_end=False), ValueError, "N_eval=None evaluates at the end of inflation and needs stop_at_end"),
    (lambda: bg.power_spectra(A, P, [6.0], X, V, N_eval="x"), ValueError, "N_eval must be None or a number"),
    (lambda: bg.power_spectra(A, P, [6.0, 8.0], X, V, N_eval=8.0), ValueError, "N_eval must be finite and > max(N_exit) = 8.0 (got 8.0)"),
    (lambda: bg.power_spectra(A, P, [6.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.power_spectra(A, P33, [6.0], X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.power_spectra(A, P, [], X, V, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before N_exit
    (lambda: bg.power_spectra(A, P, [], X, V, N_sub=0.0), ValueError, "N_exit must hold at least one e-fold count"),  # two faults: N_exit's size before N_sub
    (lambda: bg.power_spectra(A, P, [4.0], X, V, N_sub=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before N_exit's values
    (lambda: bg.power_spectra(A, P, [4.0], X, V, stop_at_end=False), ValueError, "N_exit must be finite and >= N_sub = 5.0"),  # two faults: N_exit before N_eval
    (lambda: bg.power_spectra(A, P, [6.0], [1.0, 2.0], V, N_eval=1.0), ValueError, "N_eval must be finite and > max(N_exit) = 6.0 (got 1.0)"),  # two faults: N_eval before fields
    (lambda: bg.power_spectra(A, P33, [6.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before pars
    (lambda: bg.tensor_spectra(A, P, [4.0], X, V), ValueError, "N_exit must be finite and >= N_sub = 5.0"),
    (lambda: bg.tensor_spectra(A, P, [6.0], X, V, N_eval=6.0), ValueError, "N_eval must be finite and > max(N_exit) = 6.0 (got 6.0)"),
    (lambda: bg.tensor_spectra(A, P, [6.0], X, [0.0, 0.0]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2, 2) and (2,))"),
    (lambda: bg.tensor_spectra(A, P33, [6.0], [1.0, 2.0], V, N_eval=1.0), ValueError, "N_eval must be finite and > max(N_exit) = 6.0 (got 1.0)"),  # two faults: N_eval before fields
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, 55.0, "x"), ValueError, "N_sub must be a number"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, 55.0, -1.0), ValueError, "N_sub must be finite and > 0 (got -1.0)"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, None), ValueError, "N_star must be a number"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, "x"), ValueError, "N_star must be a number"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, math.inf), ValueError, "N_star must be finite and >= 0 (got inf)"),
    (lambda: bg.spectrum_map(A, P, SS, 0, 2), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.spectrum_map(A, P13, SS, 3, 2), InflatoxShapeError, "efolds_map takes one parameter row"),
    (lambda: bg.spectrum_map(A, P, SS, 3, 2, -1.0, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before N_star
    (lambda: bg.spectrum_map(A, P, [0.0, 1.0], 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    # ---- spectra_evolution, evolution_map, transfer_from_spectra
    (lambda: bg.spectra_evolution(A, P, [6.0], [0.0], X, V, since="x"), ValueError, "since must be 'exit' or 'start' (got 'x')"),
    (lambda: bg.spectra_evolution(A, P, [6.0], "abc", X, V), ValueError, "samples must be convertible to a float64 array"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [[0.0]], X, V), InflatoxShapeError, "samples must be one-dimensional (got shape (1, 1))"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [], X, V), ValueError, "samples must hold at least one e-fold count (and fewer than 2^32)"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [1.0, 1.0], X, V), ValueError, "samples must be finite and strictly increasing"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [0.0, math.inf], X, V), ValueError, "samples must be finite and strictly increasing"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [-6.0, 0.0], X, V), ValueError, "samples since the exit must be >= -N_sub = -5.0: a mode starts N_sub e-folds before its exit (got -6.0)"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [0.0, 3.0], X, V, N_eval=8.0), ValueError, "no sample may lie beyond N_eval = 8.0 (the last one is 3.0, since='exit')"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [0.0, 9.0], X, V, N_eval=8.0, since="start"), ValueError, "no sample may lie beyond N_eval = 8.0 (the last one is 9.0, since='start')"),
    (lambda: bg.spectra_evolution(A, P, [4.0], [0.0], X, V), ValueError, "N_exit must be finite and >= N_sub = 5.0"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [0.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.spectra_evolution(A, P, [6.0], [], [1.0, 2.0], V, since="x"), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before since
    (lambda: bg.spectra_evolution(A, P, [6.0], [], X, V, since="x"), ValueError, "since must be 'exit' or 'start' (got 'x')"),  # two faults: since before samples
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [0.0], 55.0, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [0.0], None), ValueError, "N_star must be a number"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [0.0], -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, []), ValueError, "samples must hold at least one e-fold count (and fewer than 2^32)"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [-6.0]), ValueError, "samples since the exit must be >= -N_sub = -5.0: a mode starts N_sub e-folds before its exit (got -6.0)"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [1.0, 0.0]), ValueError, "samples must be finite and strictly increasing"),
    (lambda: bg.evolution_map(A, P, SS, 0, 2, [0.0]), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [], -1.0, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before N_star
    (lambda: bg.evolution_map(A, P, SS, 3, 2, [], -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before samples
    (lambda: bg.evolution_map(A, P, [0.0, 1.0], 3, 2, []), ValueError, "samples must hold at least one e-fold count (and fewer than 2^32)"),  # two faults: samples before start_stop
    (lambda: bg.transfer_from_spectra(SP, 1.5), TypeError, "'float' object cannot be interpreted as an integer"),
    (lambda: bg.transfer_from_spectra(types.SimpleNamespace(P_R=SP.P_R, P_S=SP.P_S[:1], C_RS=SP.C_RS), 0), InflatoxShapeError, "P_R, P_S and C_RS must have one shape (..., S) (got (2, 4), (1, 4) and (2, 4))"),
    (lambda: bg.transfer_from_spectra(types.SimpleNamespace(P_R=1.0, P_S=1.0, C_RS=1.0), 0), InflatoxShapeError, "P_R, P_S and C_RS must have one shape (..., S) (got (), () and ())"),
    (lambda: bg.transfer_from_spectra(SP, 4), ValueError, "ref must index one of the 4 samples (got 4)"),
    (lambda: bg.transfer_from_spectra(SP, -5), ValueError, "ref must index one of the 4 samples (got -5)"),
    # ---- observables, observables_map
    (lambda: bg.observables(A, P, [6.0], X, V, dN="x"), ValueError, "dN must be a number"),
    (lambda: bg.observables(A, P, [6.0], X, V, dN=0.0), ValueError, "dN must be finite and > 0 (got 0.0)"),
    (lambda: bg.observables(A, P, [5.25], X, V), ValueError, "N_exit - dN must be >= N_sub = 5.0"),
    (lambda: bg.observables(A, P, [6.0], X, V, N_eval=6.5), ValueError, "N_eval must be > max(N_exit) + dN = 6.5 (got 6.5)"),
    (lambda: bg.observables(A, P, [4.0], X, V), ValueError, "N_exit must be finite and >= N_sub = 5.0"),
    (lambda: bg.observables(A, P, [6.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.observables(A, P, [4.0], X, V, dN=0.0), ValueError, "dN must be finite and > 0 (got 0.0)"),  # two faults: dN before N_exit
    (lambda: bg.observables(A, P, [5.25], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before N_exit - dN
    (lambda: bg.observables_map(A, P, SS, 3, 2, 55.0, 0.5, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: bg.observables_map(A, P, SS, 3, 2, 55.0, 0.0), ValueError, "dN must be finite and > 0 (got 0.0)"),
    (lambda: bg.observables_map(A, P, SS, 3, 2, "x"), ValueError, "N_star must be a number"),
    (lambda: bg.observables_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.observables_map(A, P, SS, 3, 0), ValueError, "the grid needs at least one point per axis (got 3 x 0)"),
    (lambda: bg.observables_map(A, P, SS, 3, 2, -1.0, 0.0, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before dN
    (lambda: bg.observables_map(A, P, SS, 3, 2, -1.0, 0.0), ValueError, "dN must be finite and > 0 (got 0.0)"),  # two faults: dN before N_star
    (lambda: bg.observables_map(A, P, [0.0, 1.0], 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    # ---- delta_N, fnl_map
    (lambda: bg.delta_N(A, P, X, V, h="x"), ValueError, "h must be a number or a pair of numbers"),
    (lambda: bg.delta_N(A, P, X, V, h=[1.0, 2.0, 3.0]), InflatoxShapeError, "h must be a scalar or a pair (got shape (3,))"),
    (lambda: bg.delta_N(A, P, X, V, h=0), ValueError, "h must be positive and finite (got 0)"),
    (lambda: bg.delta_N(A, P, X, V, h=[1e-2, math.inf]), ValueError, "h must be positive and finite (got [0.01, inf])"),
    (lambda: bg.delta_N(A, P, X, V, velocity="x"), ValueError, "unknown velocity rule 'x': choose 'fixed' or 'slow_roll' (or pass derivatives_init of shape (B, 3, 3, 2))"),
    (lambda: bg.delta_N(A, P, [1.0, 2.0], V), InflatoxShapeError, "fields_init must have shape (B, 2) (got (2,))"),
    (lambda: bg.delta_N(A, P, X), ValueError, "velocity='fixed' needs derivatives_init, the centres' coordinate velocities"),
    (lambda: bg.delta_N(A, P, X, np.zeros((2, 3, 3, 3))), InflatoxShapeError, "explicit member velocities must have shape (2, 3, 3, 2) (got (2, 3, 3, 3))"),
    (lambda: bg.delta_N(A, P, X, [0.0, 0.0]), InflatoxShapeError, "derivatives_init must have shape (2, 2) or (2, 3, 3, 2) (got (2,))"),
    (lambda: bg.delta_N(A, P, X, V, H_end=[1.0, 2.0, 3.0]), ValueError, "H_end must be None, a number or an array of shape (2,)"),
    (lambda: bg.delta_N(A, P, X, V, H_end=-1.0), ValueError, "H_end must be positive and finite"),
    (lambda: bg.delta_N(A, P33, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.delta_N(A, P, [1.0, 2.0], V, h=0, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before h
    (lambda: bg.delta_N(A, P, [1.0, 2.0], V, h=0), ValueError, "h must be positive and finite (got 0)"),  # two faults: h before fields
    (lambda: bg.delta_N(A, P, [1.0, 2.0], V, velocity="x"), ValueError, "unknown velocity rule 'x': choose 'fixed' or 'slow_roll' (or pass derivatives_init of shape (B, 3, 3, 2))"),  # two faults: velocity before fields
    (lambda: bg.delta_N(A, P33, X, V, H_end=-1.0), ValueError, "H_end must be positive and finite"),  # two faults: H_end before pars
    (lambda: bg.fnl_map(A, P, SS, 3, 2, 55.0, 0), ValueError, "h must be positive and finite (got 0)"),
    (lambda: bg.fnl_map(A, P, SS, 3, 2, 55.0, 1e-2, "x"), ValueError, "unknown velocity rule 'x': choose 'fixed' or 'slow_roll' (or pass derivatives_init of shape (B, 3, 3, 2))"),
    (lambda: bg.fnl_map(A, P, SS, 3, 2, None), ValueError, "N_star must be a number"),
    (lambda: bg.fnl_map(A, P, SS, 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),
    (lambda: bg.fnl_map(A, P, SS, 0, 2), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.fnl_map(A, P, SS, 3, 2, -1.0, 0), ValueError, "h must be positive and finite (got 0)"),  # two faults: h before N_star
    (lambda: bg.fnl_map(A, P, [0.0, 1.0], 3, 2, -1.0), ValueError, "N_star must be finite and >= 0 (got -1.0)"),  # two faults: N_star before start_stop
    # ---- stochastic_efolds, stochastic_map
    (lambda: bg.stochastic_efolds(A, P, X, V, 1.5), ValueError, "realisations and seed must be integers"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, seed=1.5), ValueError, "realisations and seed must be integers"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 0), ValueError, "realisations must be in [1, 2^20] (got 0)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 2**20 + 1), ValueError, "realisations must be in [1, 2^20] (got 1048577)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, seed=-1), ValueError, "seed must be in [0, 2^64) (got -1)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, noise_scale="x"), ValueError, "noise_scale, dN_max and N_stop must be numbers"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, noise_scale=-1.0), ValueError, "noise_scale must be finite and >= 0 (got -1.0)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, dN_max=0.0), ValueError, "dN_max must be positive (got 0.0)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, N_stop=-1.0), ValueError, "N_stop must be None or a positive finite number (got -1.0)"),
    (lambda: bg.stochastic_efolds(A, P, [1.0, 2.0], V, 4), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, streams=[0.5, 1.5]), ValueError, "streams must be integers in [0, 2^32)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, streams=[-1, 0]), ValueError, "streams must be integers in [0, 2^32)"),
    (lambda: bg.stochastic_efolds(A, P, X, V, 4, streams=[0, 1, 2]), InflatoxShapeError, "streams must have shape (2,) (got (3,))"),
    (lambda: bg.stochastic_efolds(A, P33, X, V, 4), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.stochastic_efolds(A, P, [1.0, 2.0], V, 0, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before realisations
    (lambda: bg.stochastic_efolds(A, P, [1.0, 2.0], V, 0), ValueError, "realisations must be in [1, 2^20] (got 0)"),  # two faults: realisations before fields
    (lambda: bg.stochastic_efolds(A, P, [1.0, 2.0], V, 4, streams=[0.5]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before streams
    (lambda: bg.stochastic_efolds(A, P33, X, V, 4, streams=[0, 1, 2]), InflatoxShapeError, "streams must have shape (2,) (got (3,))"),  # two faults: streams before pars
    (lambda: bg.stochastic_map(A, P, SS, 3, 2, 0), ValueError, "realisations must be in [1, 2^20] (got 0)"),
    (lambda: bg.stochastic_map(A, P, [0.0, 1.0], 3, 2, 4), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),
    (lambda: bg.stochastic_map(A, P, SS, 0, 2, 4), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.stochastic_map(A, P, SS, 3, 2, 4, derivatives_init=(0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),
    (lambda: bg.stochastic_map(A, P63, SS, 3, 2, 4), InflatoxShapeError, "pars must have shape (3,) or (1, 3) (got (6, 3))"),
    (lambda: bg.stochastic_map(A, P13, SS, 3, 2, 4), InflatoxShapeError, "stochastic_map takes one parameter row"),
    (lambda: bg.stochastic_map(A, P, [0.0, 1.0], 3, 2, 0), ValueError, "realisations must be in [1, 2^20] (got 0)"),  # two faults: realisations before start_stop
    (lambda: bg.stochastic_map(A, P, [0.0, 1.0], 0, 2, 4), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),  # two faults: start_stop before N0
    (lambda: bg.stochastic_map(A, P13, SS, 3, 2, 4, derivatives_init=(0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),  # two faults: derivatives_init before the parameter row
    # ---- stochastic_distribution, stochastic_distribution_map
    (lambda: bg.stochastic_distribution(A, P, X, V, 1.5, 8, (0.0, 1.0)), ValueError, "realisations, bins, seed, first_realisation and lanes_per_point must be integers"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), lanes_per_point=64.0), ValueError, "realisations, bins, seed, first_realisation and lanes_per_point must be integers"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 0, 8, (0.0, 1.0)), ValueError, "realisations must be in [1, 2^32 - 1] (got 0)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 0, (0.0, 1.0)), ValueError, "bins must be in [1, 2^20] (got 0)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), seed=2**64), ValueError, "seed must be in [0, 2^64) (got 18446744073709551616)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), first_realisation=-1), ValueError, "first_realisation must be >= 0 and first_realisation + realisations at most 2^32 (got -1 + 4)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), first_realisation=2**32 - 3), ValueError, "first_realisation must be >= 0 and first_realisation + realisations at most 2^32 (got 4294967293 + 4)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), lanes_per_point=65), ValueError, "lanes_per_point must be None or a multiple of 64 in [64, 2^20] (got 65)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), centre="x"), ValueError, 'centre must be None or "classical" (got \'x\')'),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), noise_scale="x"), ValueError, "noise_scale and dN_max must be numbers"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), noise_scale=math.inf), ValueError, "noise_scale must be finite and >= 0 (got inf)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), dN_max=-1.0), ValueError, "dN_max must be positive (got -1.0)"),
    (lambda: bg.stochastic_distribution(A, P, [1.0, 2.0], V, 4, 8, (0.0, 1.0)), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), streams=[0.5, 1.5]), ValueError, "streams must be integers in [0, 2^32)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0), streams=[0]), InflatoxShapeError, "streams must have shape (2,) (got (1,))"),
    (lambda: bg.stochastic_distribution(A, P33, X, V, 4, 8, (0.0, 1.0)), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, "x"), ValueError, "N_range must be numbers"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, 1.0, 2.0)), InflatoxShapeError, "N_range must be (lo, hi) or have shape (2, 2) (got (3,))"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, np.ones((3, 2))), InflatoxShapeError, "N_range must be (lo, hi) or have shape (2, 2) (got (3, 2))"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (0.0, math.inf)), ValueError, "N_range must be finite (and so its width)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (-1e308, 1e308)), ValueError, "N_range must be finite (and so its width)"),
    (lambda: bg.stochastic_distribution(A, P, X, V, 4, 8, (1.0, 1.0)), ValueError, "N_range is empty: hi must be above lo"),
    (lambda: bg.stochastic_distribution(A, P, [1.0, 2.0], V, 4, 0, (1.0, 1.0)), ValueError, "bins must be in [1, 2^20] (got 0)"),  # two faults: bins before fields
    (lambda: bg.stochastic_distribution(A, P, [1.0, 2.0], V, 4, 8, (1.0, 1.0), streams=[0]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before streams
    (lambda: bg.stochastic_distribution(A, P33, X, V, 4, 8, (1.0, 1.0)), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),  # two faults: pars before N_range
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 2, 4, 0, (-1.0, 1.0)), ValueError, "bins must be in [1, 2^20] (got 0)"),
    (lambda: bg.stochastic_distribution_map(A, P, [0.0, 1.0], 3, 2, 4, 8, (-1.0, 1.0)), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 0, 4, 8, (-1.0, 1.0)), ValueError, "the grid needs at least one point per axis (got 3 x 0)"),
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 2, 4, 8, (-1.0, 1.0), derivatives_init=(0.0, 0.0, 0.0)), InflatoxShapeError, "derivatives_init must hold two velocities (got 3)"),
    (lambda: bg.stochastic_distribution_map(A, P63, SS, 3, 2, 4, 8, (-1.0, 1.0)), InflatoxShapeError, "pars must have shape (3,) or (1, 3) (got (6, 3))"),
    (lambda: bg.stochastic_distribution_map(A, P13, SS, 3, 2, 4, 8, (-1.0, 1.0)), InflatoxShapeError, "stochastic_distribution_map takes one parameter row"),
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 2, 4, 8, (1.0, -1.0)), ValueError, "N_range is empty: hi must be above lo"),
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 2, 4, 8, np.ones((5, 2))), InflatoxShapeError, "N_range must be (lo, hi) or have shape (6, 2) (got (5, 2))"),
    (lambda: bg.stochastic_distribution_map(A, P, [0.0, 1.0], 3, 2, 4, 0, (-1.0, 1.0)), ValueError, "bins must be in [1, 2^20] (got 0)"),  # two faults: bins before start_stop
    (lambda: bg.stochastic_distribution_map(A, P, [0.0, 1.0], 3, 0, 4, 8, (-1.0, 1.0)), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),  # two faults: start_stop before N1
    (lambda: bg.stochastic_distribution_map(A, P13, SS, 3, 2, 4, 8, (1.0, -1.0)), InflatoxShapeError, "stochastic_distribution_map takes one parameter row"),  # two faults: the parameter row before N_range
    (lambda: bg.stochastic_distribution_map(A, P, SS, 3, 2, 4, 8, (1.0, -1.0), derivatives_init=(0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),  # two faults: derivatives_init before N_range
    # ---- horizon_crossings, inflation_end and the calls at given wavenumbers
    (lambda: bg.horizon_crossings(A, P, "abc", X, V), ValueError, "ln_k must be convertible to a float64 array"),
    (lambda: bg.horizon_crossings(A, P, [[0.0]], X, V), InflatoxShapeError, "ln_k must be one-dimensional (got shape (1, 1))"),
    (lambda: bg.horizon_crossings(A, P, [], X, V), ValueError, "the number of wavenumbers must be in [1, 2^32) (got 0)"),
    (lambda: bg.horizon_crossings(A, P, [0.0, math.nan], X, V), ValueError, "ln_k must be finite"),
    (lambda: bg.horizon_crossings(A, P, [1.0, 0.0], X, V), ValueError, "ln_k must be strictly increasing"),
    (lambda: bg.horizon_crossings(A, P, [-2.0, -1.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # negative wavenumbers are allowed: the next check speaks
    (lambda: bg.horizon_crossings(A, P, [0.0], X, V, offset="x"), ValueError, "offset must be None, a number or an array of numbers"),
    (lambda: bg.horizon_crossings(A, P, [0.0], X, V, offset=[1.0, 2.0, 3.0]), InflatoxShapeError, "offset must be None, a scalar or have shape (2,) (got (3,))"),
    (lambda: bg.horizon_crossings(A, P, [0.0], X, V, offset=math.inf), ValueError, "offset must be finite"),
    (lambda: bg.horizon_crossings(A, P33, [0.0], X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.horizon_crossings(A, P, [], [1.0, 2.0], V, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before ln_k
    (lambda: bg.horizon_crossings(A, P, [], [1.0, 2.0], V), ValueError, "the number of wavenumbers must be in [1, 2^32) (got 0)"),  # two faults: ln_k before fields
    (lambda: bg.horizon_crossings(A, P, [0.0], [1.0, 2.0], V, offset="x"), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before offset
    (lambda: bg.horizon_crossings(A, P33, [0.0], X, V, offset=math.inf), ValueError, "offset must be finite"),  # two faults: offset before pars
    (lambda: bg.inflation_end(A, P, [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.inflation_end(A, P33, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.inflation_end(A, P, [1.0, 2.0], V, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before fields
    (lambda: bg.inflation_end(A, P33, [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before pars
    (lambda: bg.power_spectra_at_k(A, P, [1.0, 0.0], X, V), ValueError, "ln_k must be strictly increasing"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], X, V, N_sub=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], X, V, stop_at_end=False), ValueError, "N_eval=None evaluates at the end of inflation and needs stop_at_end"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], X, V, N_eval="x"), ValueError, "N_eval must be None or a number"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], X, V, N_eval=3.0), ValueError, "N_eval must be finite and > N_sub = 5.0 (got 3.0)"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.power_spectra_at_k(A, P, [0.0], X, V, offset=[1.0]), InflatoxShapeError, "offset must be None, a scalar or have shape (2,) (got (1,))"),
    (lambda: bg.power_spectra_at_k(A, P33, [0.0], X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: bg.power_spectra_at_k(A, P, [], X, V, N_sub=0.0), ValueError, "the number of wavenumbers must be in [1, 2^32) (got 0)"),  # two faults: ln_k before N_sub
    (lambda: bg.power_spectra_at_k(A, P, [0.0], [1.0, 2.0], V, N_sub=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before fields
    (lambda: bg.power_spectra_at_k(A, P, [0.0], [1.0, 2.0], V, offset=[1.0]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),  # two faults: fields before offset
    (lambda: bg.tensor_spectra_at_k(A, P, [0.0, 0.0], X, V), ValueError, "ln_k must be strictly increasing"),
    (lambda: bg.tensor_spectra_at_k(A, P, [0.0], X, V, N_eval=5.0), ValueError, "N_eval must be finite and > N_sub = 5.0 (got 5.0)"),
    (lambda: bg.tensor_spectra_at_k(A, P, [0.0], [1.0, 2.0], V, N_eval=5.0), ValueError, "N_eval must be finite and > N_sub = 5.0 (got 5.0)"),  # two faults: N_eval before fields
    (lambda: bg.observables_at_k(A, P, [0.0], X, V, dlnk="x"), ValueError, "dlnk must be a number"),
    (lambda: bg.observables_at_k(A, P, [0.0], X, V, dlnk=0.0), ValueError, "dlnk must be finite and > 0 (got 0.0)"),
    (lambda: bg.observables_at_k(A, P, [[0.0]], X, V), InflatoxShapeError, "ln_k must be one-dimensional (got shape (1, 1))"),
    (lambda: bg.observables_at_k(A, P, [0.0], [1.0, 2.0], V), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"),
    (lambda: bg.observables_at_k(A, P, [], X, V, dlnk=0.0), ValueError, "dlnk must be finite and > 0 (got 0.0)"),  # two faults: dlnk before ln_k
    (lambda: bg.observables_at_k(A, P, [], [1.0, 2.0], V), ValueError, "the number of wavenumbers must be in [1, 2^32) (got 0)"),  # two faults: ln_k before fields
    (lambda: bg.reheating_offset("x"), ValueError, "reheating_offset takes numbers"),
    (lambda: bg.reheating_offset(0.0), ValueError, "k_mpc must be finite and > 0 (got 0.0)"),
    (lambda: bg.reheating_offset(g_reh=math.inf), ValueError, "g_reh must be finite and > 0 (got inf)"),
    (lambda: bg.reheating_offset(gs_reh=-1.0), ValueError, "gs_reh must be finite and > 0 (got -1.0)"),
    (lambda: bg.reheating_offset(N_reh=-1.0), ValueError, "N_reh must be finite and >= 0 (got -1.0)"),
    (lambda: bg.reheating_offset(w_reh=-1.0 / 3.0), ValueError, "w_reh must be in (-1/3, 1] (got -0.3333333333333333)"),
    (lambda: bg.reheating_offset(0.0, N_reh=-1.0), ValueError, "k_mpc must be finite and > 0 (got 0.0)"),  # two faults: k_mpc before N_reh
    # ---- the pivot maps
    (lambda: bg.pivot_exit_map(A, P, [0.0, 1.0], 3, 2, -61.0), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),
    (lambda: bg.pivot_exit_map(A, P, SS, 0, 2, -61.0), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: bg.pivot_exit_map(A, P, SS, 3, 2, -61.0, (0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),
    (lambda: bg.pivot_exit_map(A, P, SS, 3, 2, "x"), ValueError, "A must be a number or an (N0, N1) array of numbers"),
    (lambda: bg.pivot_exit_map(A, P, SS, 3, 2, np.ones((2, 3))), InflatoxShapeError, "A must be a scalar or have shape (3, 2) (got (2, 3))"),
    (lambda: bg.pivot_exit_map(A, P, SS, 3, 2, math.nan), ValueError, "A must be finite"),
    (lambda: bg.pivot_exit_map(A, P63, SS, 3, 2, -61.0), InflatoxShapeError, "pars must have shape (3,) or (1, 3) (got (6, 3))"),
    (lambda: bg.pivot_exit_map(A, P13, SS, 3, 2, -61.0), InflatoxShapeError, "the pivot maps take one parameter row"),
    (lambda: bg.pivot_exit_map(A, P, [0.0, 1.0], 3, 2, -61.0, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before start_stop
    (lambda: bg.pivot_exit_map(A, P, [0.0, 1.0], 0, 2, -61.0), InflatoxShapeError, "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"),  # two faults: start_stop before N0
    (lambda: bg.pivot_exit_map(A, P, SS, 3, 2, "x", (0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),  # two faults: derivatives_init before A
    (lambda: bg.pivot_exit_map(A, P63, SS, 3, 2, math.nan), ValueError, "A must be finite"),  # two faults: A before the parameter rows
    (lambda: bg.pivot_observables_map(A, P, SS, 3, 2, -61.0, 0.5, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: bg.pivot_observables_map(A, P, SS, 3, 2, -61.0, 0.0), ValueError, "dlnk must be finite and > 0 (got 0.0)"),
    (lambda: bg.pivot_observables_map(A, P, SS, 3, 0, -61.0), ValueError, "the grid needs at least one point per axis (got 3 x 0)"),
    (lambda: bg.pivot_observables_map(A, P, SS, 3, 2, np.ones(6)), InflatoxShapeError, "A must be a scalar or have shape (3, 2) (got (6,))"),
    (lambda: bg.pivot_observables_map(A, P13, SS, 3, 2, -61.0), InflatoxShapeError, "the pivot maps take one parameter row"),
    (lambda: bg.pivot_observables_map(A, P, SS, 3, 2, -61.0, 0.0, 0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before dlnk
    (lambda: bg.pivot_observables_map(A, P, [0.0, 1.0], 3, 2, -61.0, 0.0), ValueError, "dlnk must be finite and > 0 (got 0.0)"),  # two faults: dlnk before start_stop
    (lambda: bg.pivot_observables_map(A, P63, SS, 3, 2, math.nan), ValueError, "A must be finite"),  # two faults: A before the parameter rows
    # ---- the special-function policy: the words of GeneralisedAL(..., sf_errors=), refused before the handle is opened
    (lambda: bg.set_sf_errors(A, "loud"), ValueError, "sf_errors must be \"raise\" or \"nan\" (got 'loud')"),
    (lambda: bg.set_sf_errors(A, None), ValueError, "sf_errors must be \"raise\" or \"nan\" (got None)"),
]
# fmt: on


def _called(case):
    return next(name for name in case[0].__code__.co_names if name in bg.__all__)


@pytest.fixture
def no_device(monkeypatch):
    def touched(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(bg, "_dylib", touched)
    monkeypatch.setattr(bg, "_crossing_dylib", touched)
    for name in dir(CompilationArtifact):
        if name.startswith("ensure_"):
            monkeypatch.setattr(CompilationArtifact, name, touched)
    return touched


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{i}-{_called(CASES[i])}")
def test_bad_arguments(no_device, case):
    call, error, message = CASES[case]
    with pytest.raises(error) as caught:
        call()
    assert type(caught.value) is error and str(caught.value) == message


def test_every_checking_function_is_in_the_table():
    """Every function of ``__all__`` that takes an artefact, and the three pure functions that check their arguments."""
    import inspect

    checking = {name for name in bg.__all__ if inspect.isfunction(getattr(bg, name)) and "artifact" in inspect.signature(getattr(bg, name)).parameters}
    checking |= {"transfer_from_spectra", "reheating_offset"}
    assert checking <= {_called(case) for case in CASES}, checking - {_called(case) for case in CASES}


def test_good_arguments_reach_the_device(no_device):
    """The shared arguments are good ones: with nothing wrong a function gets as far as the device (here an artefact whose ``ensure_*`` are
    out of reach as well)."""
    art = types.SimpleNamespace(n_fields=2, n_parameters=3, **{name: no_device for name in dir(CompilationArtifact) if name.startswith("ensure_")})
    for call in (lambda: bg.solve_eom_batch(art, P, 10, X, V), lambda: bg.efolds_map(art, P, SS, 3, 2), lambda: bg.horizon_crossings(art, P, [-1.0, 0.0], X, V),
                 lambda: bg.transfer_functions(art, P, [0.0], X, V, dq_dN=1.0), lambda: bg.pivot_observables_map(art, P, SS, 3, 2, -61.0),
                 lambda: bg.stochastic_distribution_map(art, P, SS, 3, 2, 4, 8, (-1.0, 1.0)), lambda: bg.kinematics(art, P, np.ones((2, 5)))):  # fmt: skip
        with pytest.raises(AssertionError, match="the device was touched"):
            call()
