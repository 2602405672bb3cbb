"""The C-ABI library loads and exports every symbol include/mpcg.h declares
(no compute calls: this runs on the CPU-only build box)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd", "libmpcg.so")
HDR = os.path.join(ROOT, "include", "mpcg.h")


def declared_functions():
    txt = open(HDR).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*|void|mpcg_context \*)\s*\**\s*(mpcg_\w+)\s*\(",
                                 txt, re.M)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        from oscar_mpc_planner_mr_modification_amd import _build
        _build.build_lib()
    return C.CDLL(LIB)


def test_header_declares_the_boundary():
    names = declared_functions()
    for n in ("mpcg_solve_batch_device", "mpcg_solve_batch_host", "mpcg_select_best_device",
              "mpcg_supported", "mpcg_abi_version", "mpcg_last_error", "mpcg_solve", "mpcg_context_create",
              "mpcg_context_solve", "mpcg_context_destroy", "mpcg_problem_from_map", "mpcg_lam_size"):
        assert n in names


def test_every_declared_symbol_is_exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    for n in declared_functions():
        assert n in exported, n
        assert getattr(lib, n) is not None


def test_python_binding_lists_the_same_symbols():
    from oscar_mpc_planner_mr_modification_amd.native_spec import EXPORTS
    assert set(EXPORTS) == set(declared_functions())


def test_host_only_queries(lib):
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.native_spec import problem_from_layout
    lib.mpcg_abi_version.restype = C.c_int
    assert lib.mpcg_abi_version() == 9
    for cfg in ("C1", "C2", "C3", "C4", "C5"):
        pr = problem_from_layout(config_layout(cfg))
        assert lib.mpcg_supported(C.byref(pr)) == 0, cfg
    pr = problem_from_layout(config_layout("C2"))
    pr.N = 17
    assert lib.mpcg_supported(C.byref(pr)) == -1
    pr = problem_from_layout(config_layout("C5"))
    pr.nx = 5   # scenario rows on the model without the slack state: not compiled
    assert lib.mpcg_supported(C.byref(pr)) == -1
    pr = problem_from_layout(config_layout("C3"))
    pr.nu = 2   # the bicycle model needs its slack input
    assert lib.mpcg_supported(C.byref(pr)) == -1
    pr = problem_from_layout(config_layout("C3"))
    pr.model = 0   # decomp rows on the unicycle: no instance
    assert lib.mpcg_supported(C.byref(pr)) == -1
    lib.mpcg_num_h.restype = C.c_int
    lib.mpcg_lam_size.restype = C.c_int
    pr = problem_from_layout(config_layout("C5"))
    assert lib.mpcg_num_h(C.byref(pr)) == 24 and lib.mpcg_lam_size(C.byref(pr)) == 20 * (6 + 24)
    # QP memory: per slot and lane the row's slack and multiplier, then step and dynamics multipliers
    lib.mpcg_qp_mem_size.restype = C.c_int
    pr = problem_from_layout(config_layout("C2"))   # 3 parts: 2 x 3 box slots + 6 h slots per lane
    assert lib.mpcg_qp_mem_size(C.byref(pr)) == 2 * 12 * 64 + 21 * 7 + 20 * 5
    pr.N = 17
    assert lib.mpcg_qp_mem_size(C.byref(pr)) == -1


def test_struct_layout_matches_header():
    """ctypes mirror vs the C struct: same field names in the same order."""
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgProblem
    txt = open(HDR).read()
    body = txt[txt.index("typedef struct mpcg_problem {"):txt.index("} mpcg_problem;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:int|double)\s+([^;]+);", body):
        for part in decl.split(","):
            names.append(re.sub(r"\[.*\]", "", part).strip())
    assert names == [f[0] for f in MpcgProblem._fields_]


def _fields(txt, struct):
    body = txt[txt.index(f"typedef struct {struct} {{"):txt.index(f"}} {struct};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:int|double)\s+([^;]+);", body):
        for part in decl.split(","):
            names.append(re.sub(r"\[.*\]", "", part).replace("*", "").strip())
    return names


def test_io_struct_layout_matches_header():
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgIo
    assert _fields(open(HDR).read(), "mpcg_io") == [f[0] for f in MpcgIo._fields_]


def _problem_from_map(lib, lay, drop=None, dt=0.2, iters=10):
    from oscar_mpc_planner_mr_modification_amd.native_spec import MpcgProblem
    items = [(k, v) for k, v in lay.pmap.items() if k != drop]
    names = (C.c_char_p * len(items))(*[k.encode() for k, _ in items])
    idx = (C.c_int * len(items))(*[v for _, v in items])
    lb = (C.c_double * lay.nvar)(*lay.lb)
    ub = (C.c_double * lay.nvar)(*lay.ub)
    pr = MpcgProblem()
    lib.mpcg_problem_from_map.restype = C.c_int
    lib.mpcg_problem_from_map_model.restype = C.c_int
    lib.mpcg_last_error.restype = C.c_char_p
    if lay.model_id == 0:
        rc = lib.mpcg_problem_from_map(C.byref(pr), lay.N, lay.nx, lay.npar, len(items), names, idx, lb, ub,
                                       C.c_double(dt), iters)
    else:
        rc = lib.mpcg_problem_from_map_model(C.byref(pr), lay.model_id, lay.N, lay.nx, lay.npar, len(items), names,
                                             idx, lb, ub, C.c_double(dt), iters)
    return rc, pr


@pytest.mark.parametrize("cfg", ["C1", "C2", "C3", "C4", "C5"])
def test_problem_from_parameter_map_matches_layout(lib, cfg):
    """mpcg_problem_from_map (what the C++ Solver calls on parameter_map.yaml)
    reproduces the Python layout's problem field by field."""
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.native_spec import problem_from_layout
    lay = config_layout(cfg)
    rc, pr = _problem_from_map(lib, lay)
    assert rc == 0
    ref = problem_from_layout(lay)
    for name, _ in ref._fields_:
        a, b = getattr(pr, name), getattr(ref, name)
        if hasattr(a, "__len__"):
            assert list(a) == list(b), name
        else:
            assert a == b, name


@pytest.mark.parametrize("profile", ["hpipm", "robust"])
def test_qp_profiles_agree(lib, profile):
    """mpcg_problem_set_qp_profile (libmpcg.so), native_spec.QP_PROFILES and the oracle's profiles
    set the same interior-point fields; the drop-in's default is HPIPM's"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    from oscar_mpc_planner_mr_modification_amd.native_spec import QP_FIELDS, QP_PROFILES, problem_from_layout
    lay = config_layout("C2")
    rc, pr = _problem_from_map(lib, lay)
    assert rc == 0 and pr.qp_profile == 0
    lib.mpcg_problem_set_qp_profile.restype = C.c_int
    assert lib.mpcg_problem_set_qp_profile(C.byref(pr), QP_PROFILES[profile]["qp_profile_id"]) == 0
    ref = problem_from_layout(lay, qp_profile=profile)
    orc = oracle_py.problem_from_layout(lay, qp_profile=profile)
    assert pr.qp_profile == ref.qp_profile == QP_PROFILES[profile]["qp_profile_id"]
    for f in QP_FIELDS:
        assert getattr(pr, f) == getattr(ref, f) == getattr(orc, f) == QP_PROFILES[profile][f], f
        assert oracle_py.QP_PROFILES[profile][f] == QP_PROFILES[profile][f], f
    assert lib.mpcg_problem_set_qp_profile(C.byref(pr), 7) == -1


def test_problem_from_map_reports_missing_entries(lib):
    from oscar_mpc_planner_mr_modification_amd.layouts import config_layout
    rc, _ = _problem_from_map(lib, config_layout("C2"), drop="contour")
    assert rc == -1
    assert b"contour" in lib.mpcg_last_error()
    rc, _ = _problem_from_map(lib, config_layout("C2"), drop="ellipsoid_obst_3_r")
    assert rc == -1 and b"obstacle 3" in lib.mpcg_last_error()


def test_select_best_rejects_invalid_arguments(lib):
    """mpcg_select_best_device checks its arguments before it launches, as mpcg_winner_records_device and
    mpcg_select_lowest_cost_device do: -1 with the error text set (no device call is reached)"""
    vp = C.c_void_p
    lib.mpcg_select_best_device.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_double, vp, vp,
                                            C.c_double, vp, vp, vp, vp]
    lib.mpcg_select_best_device.restype = C.c_int
    lib.mpcg_last_error.restype = C.c_char_p
    buf = (C.c_double * 8)()
    p = C.cast(buf, vp)     # stands for a device pointer: never dereferenced on these paths

    def call(S=1, G=1, N=1, xtraj=p, pobj=p, exit_code=p, best=p):
        return lib.mpcg_select_best_device(S, G, N, xtraj, pobj, exit_code, None, 0.0, None, None, 1.0, None, best,
                                           None, None)

    for kw in (dict(S=-1), dict(G=0), dict(N=0), dict(xtraj=None), dict(pobj=None), dict(exit_code=None),
               dict(best=None)):
        assert call(**kw) == -1, kw
        assert b"mpcg_select_best_device" in lib.mpcg_last_error(), kw
    # no scenes: nothing to do, the buffers may be missing
    assert call(S=0, xtraj=None, pobj=None, exit_code=None, best=None) == 0
    assert call(S=0, G=0) == -1


def test_product_path_fails_loudly_without_the_hip_library(tmp_path):
    """No CPU fallback: with libmpcg.so absent, importing the binding raises."""
    import sys

    env = dict(os.environ, MPCG_LIB=str(tmp_path / "libmpcg_absent.so"))
    code = "import oscar_mpc_planner_mr_modification_amd.native"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "not built" in r.stderr and "no CPU fallback" in r.stderr
