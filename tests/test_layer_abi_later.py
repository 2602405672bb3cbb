"""The host-side seam of the later layers: tests/test_layer_abi.py pins the key sets of
_build.LAYERS and native_spec.SIGNATURES to the first five layers, so the layers after them register in
_build.LATER_LAYERS and native_spec.LATER_SIGNATURES.  The same four-way comparison here: the functions the
public header declares, the *_EXPORTS tuple, the signature group and the dynamic symbols of libmpcg.so are
one set of names; native applies every signature; and the hashed sources are untouched.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import pytest

from oscar_mpc_planner_mr_modification_amd import _build
from oscar_mpc_planner_mr_modification_amd import native_spec as ns
from test_layer_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# public header -> (the functions it declares, the binding's tuple of them)
LATER_FUNCTIONS = {
    "mpcg_decomp.h": (["mpcg_decomp_halfspaces"], ns.DECOMP_EXPORTS),
}


def test_the_later_tables_name_the_same_layers_and_none_of_the_first():
    assert set(_build.LATER_LAYERS) == set(LATER_FUNCTIONS) == set(ns.LATER_SIGNATURES)
    assert not set(_build.LATER_LAYERS) & set(_build.LAYERS) and not set(ns.LATER_SIGNATURES) & set(ns.SIGNATURES)
    first = {n for g in ns.SIGNATURES.values() for n in g}
    assert not first & {n for g in ns.LATER_SIGNATURES.values() for n in g}
    assert set(_build.all_layers()) == set(_build.LAYERS) | set(_build.LATER_LAYERS)


@pytest.mark.parametrize("header", list(LATER_FUNCTIONS))
def test_header_binding_and_library_hold_the_same_functions(header):
    names, exports = LATER_FUNCTIONS[header]
    assert declared_functions(header) == names
    assert set(exports) == set(ns.LATER_SIGNATURES[header]) == set(names) and len(exports) == len(names)
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    lib = C.CDLL(_build.LIB)
    for n in names:
        assert n in exported, n
        assert getattr(lib, n) is not None


def test_the_build_takes_the_later_layers_in():
    srcs = _build.lib_sources()
    for layer in _build.LATER_LAYERS.values():
        for src, flags in layer["sources"].items():
            assert srcs[src] == flags and src not in _build.SOURCES
            assert os.path.exists(os.path.join(_build.CSRC, src))
        for h in layer["headers"]:
            assert h not in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, h))
    assert _build.LATER_LAYERS["mpcg_decomp.h"] == {"sources": {"mpcg_decomp.hip": ["-ffp-contract=off"]},
                                                    "headers": ["mpcg_decomp.h"]}
    assert "mpcg_wave.h" in _build.LAYER_SHARED_HEADERS and "mpcg_wave.h" not in _build.HEADERS


def test_native_applies_every_later_signature():
    from oscar_mpc_planner_mr_modification_amd import native
    n = 0
    for group in ns.LATER_SIGNATURES.values():
        for name, (restype, argtypes) in group.items():
            fn = getattr(native.lib, name)
            assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
            assert fn.restype is restype, name
            n += 1
    assert n == sum(len(v[0]) for v in LATER_FUNCTIONS.values())
    assert callable(native.decomp_halfspaces_device)


def test_decomp_structs_and_constants_mirror_the_header():
    txt = open(os.path.join(_build.INCLUDE, "mpcg_decomp.h")).read()
    for macro, value in (("MPCG_DECOMP_MAX_POINTS", ns.DECOMP_MAX_POINTS), ("MPCG_DECOMP_MAX_N", ns.DECOMP_MAX_N),
                         ("MPCG_DECOMP_MAX_ROWS", ns.DECOMP_MAX_ROWS), ("MPCG_DECOMP_EPS", ns.DECOMP_EPS)):
        line = next(l for l in txt.splitlines() if l.startswith(f"#define {macro} "))
        assert float(line.split()[2]) == value, macro
    assert [f[0] for f in ns.MpcgDecompSettings._fields_] == ["range", "deceleration"]
    assert [f[0] for f in ns.MpcgDecompIo._fields_] == ["state", "main_warm", "occ", "n_occ", "max_points"]
    assert C.sizeof(ns.MpcgDecompSettings) == 16 and C.sizeof(ns.MpcgDecompIo) == 40


def test_counter_profiles_still_match_the_hashed_sources():
    """the decomp sources are linked into libmpcg.so but are not part of source_hash()"""
    with open(os.path.join(ROOT, "profiles", "traffic_C2.json")) as fh:
        assert _build.source_hash() == json.load(fh)["source_sha256"]
