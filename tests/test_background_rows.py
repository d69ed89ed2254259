"""Device-resident rows without a GPU: the tile map of the row transpose and the plan of a call's lane passes on the CPU
(tests/background_rows_twin.cpp, a stand-alone program under the address and undefined-behaviour sanitizers), the argument checks of
``solve_eom_batch_device``, and what the library and the background object export."""

import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import workloads
from conftest import ROOT

CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_tile_map_and_pass_plan_under_sanitizers(tmp_path):
    """Every thread of every workgroup through load and then store, n in {1, 63, 64, 65, 257} x filled in {1, 7, 8, 9, 19} with
    row_base = 3, lane_off = 2 and a destination of n + 4 lanes x filled + 5 rows pre-filled with a sentinel: every element of the
    window holds its source bits (NaN payloads, -0.0), every other one the sentinel, and no access leaves the heap blocks.  Then the
    pass plan's table.  The program is linked with the sanitizers where the compiler can link them, and plainly otherwise."""
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx, "no host C++ compiler"
    exe = str(tmp_path / "background_rows_twin")
    base = [gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", f"-I{CSRC}", os.path.join(ROOT, "tests", "background_rows_twin.cpp"), "-o", exe]
    built = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600)
    sanitized = built.returncode == 0
    if not sanitized:
        print("no sanitizer runtime to link with, building without:\n" + built.stderr[-2000:])
        built = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(("sanitized: " if sanitized else "unsanitized: ") + run.stdout + run.stderr[-4000:])
    assert run.returncode == 0 and run.stdout.startswith("ok: 27 launches"), (run.stdout, run.stderr[-4000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]


def test_public_names():
    from inflatox_amd import _native, background

    assert "solve_eom_batch_device" in background.__all__ and "solve_eom_batch_device" in background.__doc__
    assert _native.EOM_HOST_SCATTER == 8 and callable(_native.InflatoxDevLib.solve_eom_device)
    assert not _native.EOM_HOST_SCATTER & (_native.EOM_STOP_AT_END | _native.EOM_FINAL_ONLY | _native.EOM_SAMPLE_T)
    _native.build_library()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "inflx_solve_eom_device"), "libinflx_hip.so lacks inflx_solve_eom_device"
    assert "inflx_solve_eom_device" in _native.SIGNATURES and len(_native.SIGNATURES["inflx_solve_eom_device"][1]) == 20
    header = open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert "INFLX_EOM_HOST_SCATTER = 8" in header


def test_bad_arguments_raise_before_torch_or_the_device(monkeypatch):
    """The errors of ``solve_eom_batch``, one by one, from both calls -- with the handle and ``import torch`` made to fail."""
    import builtins

    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    real_import = builtins.__import__

    def no_torch(name, *a, **k):
        if name == "torch" or name.startswith("torch."):
            raise AssertionError("torch was imported")
        return real_import(name, *a, **k)

    monkeypatch.setattr(background, "_dylib", no_device)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2))
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    cases = [
        (shape, dict(x=x, v=v[:2])),  # wrong shapes
        (shape, dict(x=np.zeros((3, 3)), v=np.zeros((3, 3)))),
        (shape, dict(x=np.zeros(3), v=np.zeros(3))),
        (shape, dict(p=p[:2])),
        (shape, dict(p=np.zeros((2, p.size)))),
        (shape, dict(art=three)),
        (value, dict(steps=0)),  # steps < 1
        (value, dict(steps=-4)),
        (value, dict(steps=2.5)),
        (value, dict(solver="euler")),  # unknown solver
        (value, dict(max_err=0.0)),  # non-positive max_err
        (value, dict(max_err=-1e-6)),
        (value, dict(max_err=float("nan"))),
        (value, dict(dt=0.0)),
        (value, dict(substeps=0)),
    ]
    for call in (background.solve_eom_batch, background.solve_eom_batch_device):
        for exc, kw in cases:
            kw = dict(kw)
            args = (kw.pop("art", art), kw.pop("p", p), kw.pop("steps", 5), kw.pop("x", x), kw.pop("v", v))
            with pytest.raises(exc) as err:
                call(*args, **kw)
            assert err.type is exc, (call.__name__, kw, err.type)
    # the same message from both, and the same check first when two arguments are wrong (the checks run in the same order)
    for kw in (dict(steps=0, solver="euler"), dict(max_err=-1.0, solver="euler"), dict(solver="euler", dt=-1.0)):
        said = []
        for call in (background.solve_eom_batch, background.solve_eom_batch_device):
            kw2 = dict(kw)
            with pytest.raises(ValueError) as err:
                call(art, p, kw2.pop("steps", 5), x, v[:2], **kw2)
            said.append(str(err.value))
        assert said[0] == said[1], said
    # good arguments get as far as torch
    with pytest.raises(AssertionError, match="torch was imported"):
        background.solve_eom_batch_device(art, p, 5, x, v)


def _elf_symbols(path):
    """{name: (value, size, section index)} of the ELF64 symbol tables of ``path``, and its section headers (type, address, offset)."""
    data = open(path, "rb").read()
    assert data[:4] == b"\x7fELF" and data[4] == 2 and data[5] == 1, "not a little-endian ELF64 file"
    shoff, shentsize, shnum = struct.unpack_from("<Q", data, 0x28)[0], *struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + k * shentsize) for k in range(shnum)]
    symbols = {}
    for sh in sections:
        if sh[1] not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
            continue
        strtab = sections[sh[6]]
        for off in range(sh[4], sh[4] + sh[5], sh[9]):
            name, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", data, off)
            end = data.index(b"\0", strtab[4] + name)
            symbols[data[strtab[4] + name : end].decode()] = (value, size, shndx)
    return data, sections, symbols


def test_background_object_exports_layout_5_and_the_transpose_kernel():
    """The cross-compiled hyperbolic background object: INFLX_BG_ABI holds 5 and inflx_bg_rows_transpose is a kernel of it (a function
    symbol and its kernel descriptor), beside the kernels it had."""
    _, art = workloads.artifact_for("hyperbolic")
    data, sections, symbols = _elf_symbols(art.ensure_background())
    assert "INFLX_BG_ABI" in symbols, sorted(symbols)
    value, size, shndx = symbols["INFLX_BG_ABI"]
    sec = sections[shndx]
    assert size == 4 and sec[1] == 1, (size, sec)  # SHT_PROGBITS: the value is in the file
    (abi,) = struct.unpack_from("<I", data, sec[4] + value - sec[3])
    assert abi == 5, abi
    for kernel in ("inflx_bg_rows_transpose", "inflx_bg_init", "inflx_bg_advance_rkf_rows", "inflx_bg_advance_rk4_rows", "inflx_bg_advance_rkf_sampled"):
        assert kernel in symbols and kernel + ".kd" in symbols, kernel
    from inflatox_amd.compiler import _BACKGROUND_SOURCES

    assert "inflx_background_rows.h" in _BACKGROUND_SOURCES
    abi_header = open(os.path.join(CSRC, "inflx_background_abi.h")).read()
    assert "#define INFLX_BG_ABI_VERSION 5" in abi_header
