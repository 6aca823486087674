"""gsplatloc_amd/stages.py against include/gsloc_hip.h, without a GPU and without the library: every caller hands its
arguments to its entry point in the header's order -- a transposed, dropped or doubled argument fails here, not as a
launch error on a GPU."""
import inspect
import types

import pytest

from gsplatloc_amd import stages
from tests.test_abi import prototypes

CALLERS = ["fused_project", "fused_bin", "fused_raster_fwd", "fused_raster_bwd", "fused_project_bwd", "fused_absgrad",
           "tiny_raster_bwd", "long_sort", "long_raster_fwd", "long_raster_bwd"]
SIZED = {"ws_bytes": "ws", "long_ws_bytes": "long_ws"}  # sizes the caller takes from the workspace tensor


class _Tensor:
    """Stands in for a tensor: its own device pointer and its own size."""

    def __init__(self, k):
        self.k = k

    def data_ptr(self):
        return 1000 + self.k

    def numel(self):
        return 5000 + self.k


@pytest.mark.parametrize("caller", CALLERS)
def test_caller_passes_the_headers_argument_list(caller, repo_root, monkeypatch):
    name = "gsl_" + caller
    header = prototypes(repo_root)[name][1]
    fn = getattr(stages, caller)
    sig = inspect.signature(fn).parameters
    # the Python parameters are the header's, by name and in its order, less the sizes and the stream; what has a default
    # is keyword-only and defaults to NULL / 0
    in_header = [n for _, n in header]
    assert in_header[-1] == "stream"
    assert sorted(sig) == sorted(n for n in in_header[:-1] if n not in SIZED), caller
    for kind in (inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY):
        mine = [n for n, p in sig.items() if p.kind is kind]
        assert mine == [n for n in in_header if n in mine], (caller, kind)
    for n, p in sig.items():
        optional = p.default is not inspect.Parameter.empty
        assert optional == (p.kind is inspect.Parameter.KEYWORD_ONLY), (caller, n)
        assert p.kind is not inspect.Parameter.VAR_POSITIONAL and p.kind is not inspect.Parameter.VAR_KEYWORD
        if optional:
            assert p.default is None or (p.default == 0 and not isinstance(p.default, bool)), (caller, n, p.default)

    recorded, checked = [], []
    stream = object()
    lib = types.SimpleNamespace(**{name: lambda *a: recorded.append(a) or 0})
    monkeypatch.setattr(stages, "load_library", lambda: lib)
    monkeypatch.setattr(stages, "current_stream", lambda: stream)
    monkeypatch.setattr(stages, "check", lambda status, what: checked.append((status, what)))

    def sentinel(k, c_type):
        return _Tensor(k) if "*" in c_type else 100 + k  # distinct for every parameter

    def expected(args):
        """What the entry point must receive for these Python arguments (absent: the NULL / 0 default)."""
        out = []
        for c_type, n in header:
            if n == "stream":
                out.append(stream)
            elif n in SIZED:
                out.append(args[SIZED[n]].numel())
            elif n not in args:
                out.append(None if "*" in c_type else 0)
            else:
                out.append(args[n].data_ptr() if "*" in c_type else args[n])
        return out

    every = {n: sentinel(k, c_type) for k, (c_type, n) in enumerate(header) if n in sig}
    required = {n: v for n, v in every.items() if sig[n].default is inspect.Parameter.empty}
    assert len(required) < len(every), caller  # (each of the ten has a mode that is off by default)
    for args in (every, required):
        del recorded[:], checked[:]
        positional = [args[n] for n, p in sig.items() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        keywords = {n: args[n] for n, p in sig.items() if p.kind is inspect.Parameter.KEYWORD_ONLY and n in args}
        fn(*positional, **keywords)
        assert checked == [(0, name)]
        assert len(recorded) == 1 and len(recorded[0]) == len(header)
        got, want = list(recorded[0]), expected(args)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g is w or (g == w and not isinstance(g, bool)), (caller, i, header[i][1], g, w)
