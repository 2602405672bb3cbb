"""The host-side seam of the open tables: tests/test_layer_abi.py and
tests/test_layer_abi_later.py pin the key sets of the first two pairs of tables, so the layers after them register
in _build.OPEN_LAYERS and native_spec.OPEN_SIGNATURES.  This test pins no key set: it holds every entry it finds
to the four-way comparison (the functions the public header declares, the *_EXPORTS tuple, the signature group
and the dynamic symbols of libmpcg.so are one set of names), checks that the scenario sampler is among them, that
native applies every signature, and that the hashed sources are untouched.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import pytest

from oscar_mpc_planner_mr_modification_amd import _build
from oscar_mpc_planner_mr_modification_amd import native_spec as ns
from test_layer_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _exports_tuple(header):
    """the binding's tuple of a header's functions: <LAYER>_EXPORTS for mpcg_<layer>.h"""
    return getattr(ns, header[len("mpcg_"):-len(".h")].upper() + "_EXPORTS")


def test_the_open_tables_name_the_same_layers_and_none_of_the_pinned():
    assert set(_build.OPEN_LAYERS) == set(ns.OPEN_SIGNATURES)
    assert "mpcg_scenario.h" in _build.OPEN_LAYERS
    assert not set(_build.OPEN_LAYERS) & set(_build.all_layers())
    assert not set(ns.OPEN_SIGNATURES) & (set(ns.SIGNATURES) | set(ns.LATER_SIGNATURES))
    pinned = {n for t in (ns.SIGNATURES, ns.LATER_SIGNATURES) for g in t.values() for n in g}
    assert not pinned & {n for g in ns.OPEN_SIGNATURES.values() for n in g}
    assert set(_build.linked_layers()) == set(_build.all_layers()) | set(_build.OPEN_LAYERS)
    assert set(_build.all_layers()) == set(_build.LAYERS) | set(_build.LATER_LAYERS)


@pytest.mark.parametrize("header", list(_build.OPEN_LAYERS))
def test_header_binding_and_library_hold_the_same_functions(header):
    names = declared_functions(header)
    exports = _exports_tuple(header)
    assert names and set(exports) == set(ns.OPEN_SIGNATURES[header]) == set(names) and len(exports) == len(names)
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    lib = C.CDLL(_build.LIB)
    for n in names:
        assert n in exported, n
        assert getattr(lib, n) is not None


def test_the_scenario_header_declares_its_three_entry_points():
    assert declared_functions("mpcg_scenario.h") == ["mpcg_scenario_advance", "mpcg_scenario_sample_prepare",
                                                     "mpcg_scenario_samples"]
    assert set(ns.SCENARIO_EXPORTS) == set(declared_functions("mpcg_scenario.h"))


def test_the_build_takes_the_open_layers_in():
    srcs = _build.lib_sources()
    for header, layer in _build.OPEN_LAYERS.items():
        assert os.path.exists(os.path.join(_build.INCLUDE, header))
        for src, flags in layer["sources"].items():
            assert srcs[src] == flags and src not in _build.SOURCES
            assert os.path.exists(os.path.join(_build.CSRC, src))
        for h in layer["headers"]:
            assert h not in _build.HEADERS and os.path.exists(os.path.join(_build.CSRC, h))
    assert _build.OPEN_LAYERS["mpcg_scenario.h"] == {"sources": {"mpcg_scenario.hip": ["-ffp-contract=off"]},
                                                     "headers": ["mpcg_scenario.h"]}


def test_native_applies_every_open_signature():
    from oscar_mpc_planner_mr_modification_amd import native
    for group in ns.OPEN_SIGNATURES.values():
        for name, (restype, argtypes) in group.items():
            fn = getattr(native.lib, name)
            assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
            assert fn.restype is restype, name
    for f in ("scenario_sample_prepare_device", "scenario_samples_device", "scenario_advance_device"):
        assert callable(getattr(native, f)), f


def test_scenario_structs_and_constants_mirror_the_header():
    txt = open(os.path.join(_build.INCLUDE, "mpcg_scenario.h")).read()
    for macro, value in (("MPCG_SCENARIO_MAX_SAMPLES", ns.SCENARIO_MAX_SAMPLES),
                         ("MPCG_SCENARIO_MAX_OBS", ns.SCENARIO_MAX_OBS), ("MPCG_SCENARIO_MAX_N", ns.SCENARIO_MAX_N),
                         ("MPCG_SCENARIO_MAX_ROWS", ns.SCENARIO_MAX_ROWS)):
        line = next(l for l in txt.splitlines() if l.startswith(f"#define {macro} "))
        assert int(line.split()[2]) == value, macro
    for const in (ns.SCENARIO_MIX_C1, ns.SCENARIO_MIX_C2, ns.SCENARIO_MIX_M1, ns.SCENARIO_MIX_M2):
        assert f"0x{const:016X}" in txt
    assert [f[0] for f in ns.MpcgScenarioSampleIo._fields_] == [
        "stage_params", "state", "main_warm", "obst", "obst_meta", "bank", "batch_idx", "n_obs", "n_per", "n_batches",
        "seed", "draw", "robot_radius", "deceleration"]
    assert [f[0] for f in ns.MpcgScenarioStepIo._fields_] == ["best", "exit_code", "xtraj", "utraj", "lam_out",
                                                             "state_next", "deceleration"]
    # 7 pointers, 3 ints (+ padding), 2 unsigned long long, 2 doubles; 6 pointers and a double
    assert C.sizeof(ns.MpcgScenarioSampleIo) == 104 and C.sizeof(ns.MpcgScenarioStepIo) == 56
    assert ns.MpcgScenarioSampleIo.seed.offset == 72 and ns.MpcgScenarioSampleIo.robot_radius.offset == 88


def test_argument_checks_report_through_last_error():
    """the entry points refuse what the header lists before any launch (host pointers never reach a kernel)"""
    from oscar_mpc_planner_mr_modification_amd import native
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout, safe_horizon_layout
    pr = native.problem_from_layout(safe_horizon_layout(N=10, n_constraints=4))
    one = C.c_void_p(8)      # a non-null address; no call below launches

    def io(**kw):
        d = dict(stage_params=8, state=8, main_warm=None, obst=8, obst_meta=8, bank=8, batch_idx=None, n_obs=3,
                 n_per=7, n_batches=2, seed=1, draw=0, robot_radius=0.3, deceleration=3.0)
        d.update(kw)
        return ns.MpcgScenarioSampleIo(*d.values())

    def prepare(pr_, sio, P=4):
        return native.lib.mpcg_scenario_sample_prepare(C.byref(pr_), 1, P, C.byref(sio), one, one, one, None)

    for bad, text in ((io(n_obs=65), "n_obs"), (io(n_obs=0), "n_obs"), (io(n_per=0), "M"), (io(n_obs=64, n_per=33), "M"),
                      (io(n_batches=0), "n_batches"), (io(bank=None), "invalid"), (io(state=None), "invalid")):
        assert prepare(pr, bad) == -1 and text in native.last_error(), native.last_error()
    assert prepare(pr, io(), P=0) == -1
    tmpc = native.problem_from_layout(config_layout("C2"))
    assert prepare(tmpc, io()) == -1 and "scenario rows" in native.last_error()
    assert native.lib.mpcg_scenario_samples(C.byref(pr), 1, 4, C.byref(io(n_batches=0)), one, None) == -1
    sio = ns.MpcgScenarioStepIo(None, 8, 8, 8, None, 8, 3.0)
    assert native.lib.mpcg_scenario_advance(C.byref(pr), 1, 4, C.byref(sio), one, None, None) == -1
    assert native.lib.mpcg_scenario_advance(C.byref(tmpc), 1, 4, C.byref(sio), one, None, None) == -1
    # an empty batch is no error and launches nothing
    assert native.lib.mpcg_scenario_sample_prepare(C.byref(pr), 0, 4, C.byref(io()), one, one, one, None) == 0


def test_counter_profiles_still_match_the_hashed_sources():
    """the scenario sources are linked into libmpcg.so but are not part of source_hash()"""
    with open(os.path.join(ROOT, "profiles", "traffic_C2.json")) as fh:
        assert _build.source_hash() == json.load(fh)["source_sha256"]
    for layer in _build.OPEN_LAYERS.values():
        assert not set(layer["sources"]) & set(_build.SOURCES) and not set(layer["headers"]) & set(_build.HEADERS)
