"""The hand-written arithmetic of csrc/inflx_device_math.h against the operations it replaces, on the device
(tests/device_math_probe.hip, a stand-alone program built with the kernels' own compiler flags):

  * inflx_ipow<N>, inflx_hpow<N>, their reciprocals and the stand-alone x**(-1/2) form have the class (NaN, inf, zero, finite) and
    the sign of OCML's pow(x, e) at zeros, infinities, NaN, denormals, negative bases and bases whose power over- or underflows,
    and lie within (N-1) resp. ((N-1)/2 + 1) roundings (one more for a reciprocal) of powl's value where nothing on the way is
    denormal; inflx_hpow_checked<N> returns the bits of inflx_hpow<N> wherever its guard accepts; the guard refuses zeros,
    denormals, infinities and NaN and accepts at least every argument with 2^-500 <= |x| <= 2^500;
  * inflx_div_by_hoisted (with inflx_recip), inflx_shared_reciprocal + inflx_div_by_shared, inflx_div_by_hoisted_inline and
    inflx_div_by_hoisted_in_range return the bits of the compiler's a / b wherever they accept a pair, and refuse every pair with
    a zero, denormal, infinite or NaN numerator, denominator or quotient and every denominator outside their guard.

Every operand set runs twice: in random order and sorted by operand class (wave-uniform: the ballot branch of the inline
quotient).  The program's report of a GPU run is kept in profiles/device_math_probe.txt."""

import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_power_rewrites_and_fast_divisions_equal_what_they_replace(gpu_lib, tmp_path):
    from inflatox_amd.compiler import Compiler, hipcc_path

    exe = tmp_path / "device_math_probe"
    # the kernels' own flags, as an executable instead of a code object
    flags = [f for f in Compiler.default_hipcc_flags if f not in ("--genco", "--no-gpu-bundle-output")]
    assert "-fno-fast-math" in flags and "-ffp-contract=on" in flags and len(flags) == len(Compiler.default_hipcc_flags) - 2
    csrc = os.path.join(ROOT, "inflatox_amd", "csrc")
    subprocess.run([hipcc_path(), *flags, f"-I{csrc}", os.path.join(ROOT, "tests", "device_math_probe.hip"), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe), "20"], capture_output=True, text=True, timeout=300)
    print(proc.stdout)
    assert proc.returncode == 0, proc.stdout[-6000:] + proc.stderr
    assert "powers: 0 mismatches" in proc.stdout and "divisions: 0 mismatches" in proc.stdout and "device_math_probe: ok" in proc.stdout, proc.stdout[-6000:]
