"""CPU-side checks of the C-ABI boundary: the library builds/loads and exports exactly
the symbols include/gsloc_hip.h declares; argument validation returns error codes
without touching a GPU."""
import os
import re

from gsplatloc_amd import _lib


def _declared(repo_root):
    txt = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gsl_[a-z_0-9]+)\s*\(", txt)))


def prototypes(repo_root):
    """Every prototype of include/gsloc_hip.h: {name: (return type, [(parameter type, parameter name), ...])}, the types
    as C text without the parameter's name (``const float*``, ``int64_t``)."""
    txt = open(os.path.join(repo_root, "include", "gsloc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    out = {}
    for stmt in txt.split(";"):
        m = re.search(r"([\w\s\*]+?)\b(gsl_[a-z_0-9]+)\s*\((.*)\)\s*$", stmt.split("{")[-1], flags=re.S)
        if not m:
            continue
        params = [] if m.group(3).strip() == "void" else [
            re.fullmatch(r"\s*(.*?)\s*(\w+)\s*", p, flags=re.S).groups() for p in m.group(3).split(",")]
        out[m.group(2)] = (" ".join(m.group(1).split()), [(" ".join(t.split()), n) for t, n in params])
    return out


def _ctype(c_type):
    """The ctypes type the binding uses for a C type of the header: every pointer travels as void* (a returned string
    as char*), scalars as themselves."""
    import ctypes

    if "*" in c_type:
        return ctypes.c_char_p if "char" in c_type else ctypes.c_void_p
    return {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "uint32_t": ctypes.c_uint32}[c_type]


def test_header_and_binding_agree(repo_root):
    """_lib._SIGNATURES against the header: the same functions, and for each the same return type and the same
    parameter types in the same number and order."""
    assert _declared(repo_root) == _lib.exported_symbols()
    protos = prototypes(repo_root)
    assert sorted(protos) == _lib.exported_symbols()
    for name, (ret, params) in protos.items():
        res, args = _lib._SIGNATURES[name]
        assert res is _ctype(ret), (name, ret, res)
        assert len(args) == len(params), (name, len(args), len(params))
        for i, ((c_type, pname), arg) in enumerate(zip(params, args)):
            assert arg is _ctype(c_type), (name, i, pname, c_type, arg)


def test_headers_are_plain_c(repo_root):
    """The boundary is a C ABI: both headers must compile as C99 without any HIP / C++ / torch type."""
    import shutil
    import subprocess

    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the image"
    for h in ("gsloc_hip.h", "gsloc_icp.h"):
        res = subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                              os.path.join(repo_root, "include", h)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr


def test_library_exports_every_symbol(repo_root):
    if not os.path.exists(_lib.library_path()):
        _lib.build_library()
    lib = _lib.load_library()
    for name in _declared(repo_root):
        assert hasattr(lib, name), name
    # ... and nothing else under the library's prefix: a function one source file defines for another is not part of the
    # ABI and must not be reachable as if it were (a C symbol links against any prototype, right or wrong)
    import subprocess

    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    res = subprocess.run([readelf, "--dyn-syms", "--wide", _lib.library_path()], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    defined = {ln.split()[-1] for ln in res.stdout.splitlines() if len(ln.split()) == 8 and ln.split()[6] != "UND"}
    exported = sorted(n for n in defined if n.startswith("gsl_"))
    assert exported == _declared(repo_root), sorted(set(exported) ^ set(_declared(repo_root)))
    assert lib.gsl_version().decode().startswith("gsloc_hip")
    assert lib.gsl_status_string(-2).decode() == "workspace too small"


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib.load_library()
    # null pointers / bad sizes are caught on the host before any launch
    assert lib.gsl_project_fwd(None, None, None, None, None, 5, 64, 48, 0.3, 0.01, 1e10, 0.0, None, None, None, None,
                               None, None) == -1
    assert lib.gsl_project_fwd(None, None, None, None, None, 5, 0, 48, 0.3, 0.01, 1e10, 0.0, None, None, None, None,
                               None, None) == -1
    assert lib.gsl_rasterize_fwd(None, None, None, None, None, 7, 64, 48, 16, 4, 3, 0, 3, None, None, 0, None, None,
                                 None, None, None) == -1
    assert lib.gsl_isect_count(None, None, 0, 16, 4, 3, 0, 4, None, None, None, None, 0, None) == -1  # ty1 > tile_h
    assert lib.gsl_sh_fwd(4, None, None, None, 1, 25, None, None) == -1
    # more Gaussians than the packed gradient rows can address with 32-bit byte offsets (include/gsloc_hip.h, "Limits"):
    # means, quats, scales, opacities, colors, sh_degree, K_sh, viewmat, K, N, width, height, eps2d, near, far,
    # radius_clip, antialiased, tile_w, tile_h, ty0, ty1, then 17 pointers / sizes
    assert lib.gsl_fused_project(None, None, None, None, None, 1, 4, None, None, (1 << 26) + 1, 64, 48, 0.3, 0.01, 1e10,
                                 0.0, 0, 4, 3, 0, 3, None, None, None, None, None, None, None, None, None, 0, None, None,
                                 0, None, None, None) == -1
    assert lib.gsl_project_bwd_ws_bytes(1000) == 4 * 12 * 4
    # tile-sort launch counters (host-side): one per kernel, -1 for anything else
    assert [lib.gsl_dev_tile_sort_launches(v) >= 0 for v in range(3)] == [True] * 3
    assert lib.gsl_dev_tile_sort_launches(3) == -1 and lib.gsl_dev_tile_sort_launches(-1) == -1
    assert lib.gsl_isect_ws_bytes(100) == 800


def test_ops_fail_loudly_without_gpu_tensors():
    import pytest
    import torch

    import gsplatloc_amd as A

    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    m = torch.zeros(4, 3)
    with pytest.raises(AssertionError, match="no CPU path"):
        A.fully_fused_projection(m, None, torch.zeros(4, 4), torch.zeros(4, 3), torch.eye(4)[None], torch.eye(3)[None],
                                 32, 32)
