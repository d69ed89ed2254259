"""csrc/inflx_sf.h at its seams, limits and tiny arguments, on the device: the table of tests/special_cases.py through
tests/sf_probe.hip -- a stand-alone gfx950 program built with the kernels' own flags (-ffp-contract=on, OCML underneath, the long
routines as noinline device functions called from diverged lanes) -- and through the verdict the host suite uses
(tests/test_special_edges.py).  One build and one run for the module; the report of a GPU run is kept in
profiles/special_edges_probe.txt.  Then the refusal bit and a NaN argument through the product path."""

import os
import struct
import subprocess

import numpy as np
import pytest
import special_cases as sc
from test_special_edges import COUNTS
from test_special_functions import sf  # noqa: F401  (the host build of the header: the 2F0 seams are looked for on it)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(gpu_lib, sf, tmp_path_factory):  # noqa: F811
    from inflatox_amd.compiler import Compiler, hipcc_path

    table = sc.table(sf)
    tmp = tmp_path_factory.mktemp("sf_probe")
    exe, case_file = tmp / "sf_probe", tmp / "cases.txt"
    flags = [f for f in Compiler.default_hipcc_flags if f not in ("--genco", "--no-gpu-bundle-output")]
    assert "-fno-fast-math" in flags and "-ffp-contract=on" in flags and len(flags) == len(Compiler.default_hipcc_flags) - 2
    csrc = os.path.join(ROOT, "inflatox_amd", "csrc")
    subprocess.run([hipcc_path(), *flags, f"-I{csrc}", os.path.join(ROOT, "tests", "sf_probe.hip"), "-o", str(exe)], check=True)
    hexbits = lambda v: struct.pack(">d", v).hex()
    with open(case_file, "w") as f:
        f.write(f"{len(table.cases)}\n")
        for c in table.cases:
            f.write(f"{sc.FID[c.fn]} {c.n} {hexbits(c.p[0])} {hexbits(c.p[1])} {hexbits(c.p[2])} {hexbits(c.x)} {c.group}\n")
    proc = subprocess.run([str(exe), str(case_file)], capture_output=True, text=True, timeout=120)
    assert proc.returncode in (0, 1), proc.stdout[-3000:] + proc.stderr[-3000:]  # (1: the two passes differ -- a test of its own)
    ordered, shuffled = np.zeros(len(table.cases)), np.zeros(len(table.cases))
    status, status_shuffled, differences = [None] * len(table.groups), [None] * len(table.groups), None
    seen = 0
    for line in proc.stdout.splitlines():
        w = line.split()
        if w[0] == "R":
            ordered[int(w[1])] = struct.unpack(">d", bytes.fromhex(w[2]))[0]
            shuffled[int(w[1])] = struct.unpack(">d", bytes.fromhex(w[3]))[0]
            seen += 1
        elif w[0] == "S":
            status[int(w[1])], status_shuffled[int(w[1])] = (int(w[2]), int(w[3])), (int(w[4]), int(w[5]))
        elif w[0] == "DIFFERENCES":
            differences = int(w[1])
    assert seen == len(table.cases) and None not in status and differences is not None, proc.stdout[-3000:]
    verdicts = sc.judge(table, ordered, status, device=True)
    text = sc.report(table, verdicts, "csrc/inflx_sf.h on the device (tests/sf_probe.hip, hipcc -ffp-contract=on, OCML) against mpmath")
    text += f"\nbits that differ between the pass in table order and the shuffled pass: {differences}"
    print(text)
    if os.environ.get("INFLX_TEST_REPORT_DIR"):  # (manual runs: keeps the report, for profiles/special_edges_probe.txt)
        with open(os.path.join(os.environ["INFLX_TEST_REPORT_DIR"], "special_edges_probe.txt"), "w") as f:
            f.write(text + "\n")
    same = np.array_equal(ordered.view(np.uint64), shuffled.view(np.uint64)) and status == status_shuffled
    return table, verdicts, status, differences, same


def test_the_device_ran_every_case(probe):
    table, verdicts, _, _, _ = probe
    assert table.counts() == COUNTS
    assert len(verdicts) == len(table.cases) and all(v.rule in sc.RULES for v in verdicts)
    assert not [c for c, v in zip(table.cases, verdicts) if v.rule == "declined" and not c.decline_ok]
    assert not [c for c, v in zip(table.cases, verdicts) if v.rule in sc.LENIENT and c.check != "budget"]


@pytest.mark.parametrize("family", sc.FAMILIES)
def test_header_on_the_device(probe, family):
    table, verdicts, status, _, _ = probe
    bad = sc.failures(table, verdicts, family) + sc.status_failures(table, status, family)
    assert not bad, f"{len(bad)} of the {family} cases fail:\n" + "\n".join(bad[:60])


def test_table_order_and_shuffled_order_agree_bit_for_bit(probe):
    _, _, _, differences, same = probe
    assert differences == 0 and same


def _probe_model(kind):
    """the model of tests/test_special_gpu.py's real-order probe: same name and expression, so the same cached artefact"""
    import sympy
    from inflatox_amd import Compiler, InflationModelBuilder
    from inflatox_amd.consistency_conditions import InflationCondition

    phi, theta, nu = sympy.symbols("phi theta nu")
    fn_sym = {"J": sympy.besselj, "Y": sympy.bessely, "I": sympy.besseli, "K": sympy.besselk}[kind]
    model = InflationModelBuilder.new([phi, theta], [[1, 0], [0, 1]], fn_sym(nu, phi), model_name=f"probe_{kind}nu", init_sympy_printing=False, silent=True, assertions=False, simplify=False).build()
    art = Compiler(model, silent=True, link_gsl=True).compile()
    return InflationCondition(art, validate_basis=False)


def test_a_refusal_fails_the_call_with_its_own_code(gpu_lib):
    """J_nu with nu = 2e7: every order the potential and its derivatives need (nu, nu +- 1, nu +- 2) is declined, none is outside
    the domain -- the error carries 0X11 (the reference has no such case: GSL's own are ELOSS / EMAXITER), and with sf_errors="nan"
    the values are NaN and the status word holds INFLX_SF_EDECLINED alone, once."""
    cond = _probe_model("J")
    pts = np.array([[1.0, 0.0], [2.5, 0.0]])
    with pytest.raises(gpu_lib.InflatoxSpecialFunctionError, match="ERRCODE 0X11"):
        cond.dylib.sweep_on_trajectory(gpu_lib.OP_RAW, np.array([2e7]), pts)
    cond.dylib.set_sf_errors("nan")
    got = cond.dylib.sweep_on_trajectory(gpu_lib.OP_RAW, np.array([2e7]), pts)
    assert np.isnan(got[:, [0, 1, 4]]).all()  # V, its second derivative in phi, |dV|^2 (the derivatives in theta are 0 whatever V is)
    assert cond.dylib.sf_status() == gpu_lib.SF_EDECLINED and cond.dylib.sf_status() == 0


def test_a_nan_argument_is_no_domain_error_in_a_model(gpu_lib):
    """K_0(phi) with phi = NaN at one point of a trajectory: NaN there, no bit in the status word, no exception under the
    default policy (the model of tests/test_special_gpu.py's domain-error test: same name and expression)."""
    import sympy
    from inflatox_amd import Compiler, InflationModelBuilder
    from inflatox_amd.consistency_conditions import GeneralisedAL, InflationCondition

    phi, theta, m = sympy.symbols("phi theta m")
    potential = m**2 * (3 + sympy.besselk(0, phi) + sympy.Rational(1, 10) * sympy.cos(theta) * phi)
    model = InflationModelBuilder.new([phi, theta], [[1, 0], [0, phi**2 + 1]], potential, model_name="k0_domain", init_sympy_printing=False, silent=True, assertions=False, simplify=False).build()
    art = Compiler(model, silent=True, link_gsl=True).compile()
    al = GeneralisedAL.__new__(GeneralisedAL)  # (without the constructor's basis check at random points: some lie outside K_0's domain)
    InflationCondition.__init__(al, art, validate_basis=False)
    assert al.dylib.uses_gsl
    pts = np.stack([np.linspace(0.5, 5.0, 40), np.full(40, 0.3)], axis=1)
    pts[7, 0] = np.nan
    out = al.complete_analysis_ot(np.array([1.1]), pts, progress=False)  # the default policy: a domain error would raise here
    assert all(np.isnan(a[7]) for a in out)
    assert all(np.isfinite(a[np.arange(40) != 7]).any() for a in out[1:3])
    raw = al.dylib.sweep_on_trajectory(gpu_lib.OP_RAW, np.array([1.1]), pts)
    assert np.isnan(raw[7]).all() and np.isfinite(raw[np.arange(40) != 7]).all()
    assert al.dylib.sf_status() == 0
