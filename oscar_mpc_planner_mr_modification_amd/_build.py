"""In-tree build of the HIP backend (libmpcg.so, gfx950) and of the C++
drop-in `MPCPlanner::Solver` shim.  Outputs stay inside the package directory
(git-ignored, but they travel to the GPU box with the snapshot)."""
from __future__ import annotations

import os
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB = os.path.join(PKG, "libmpcg.so")
ARCH = os.environ.get("MPCG_OFFLOAD_ARCH", "gfx950")

# source -> extra flags.  The producers are compiled without floating-point
# contraction so that they agree bit for bit with the host restatement.
SOURCES = {"mpcg_kernels.hip": [], "mpcg_prepare.hip": ["-ffp-contract=off"],
           # built-in kernel instances, one translation unit per family (compiled in parallel)
           "mpcg_inst_tmpc20.hip": [], "mpcg_inst_tmpc30.hip": [], "mpcg_inst_shmpc.hip": [],
           "mpcg_inst_bicycle.hip": [], "mpcg_inst_road.hip": []}
HEADERS = ["mpcg_device.h", "mpcg_sqp.h", "mpcg_sqp_body.inc", "mpcg_prepare.h", "mpcg_braking.h", "mpcg_bicycle.h",
           "mpcg_instance.h", "mpcg_tail.h"]
# the layers around the SQP kernel, by public header under include/ (multi-robot fleet, reference-path
# tracking, guidance, active-solve compaction, road-boundary halfspaces): linked into libmpcg.so but kept
# out of SOURCES / HEADERS, whose source_hash() is the identity the committed counter profiles
# (profiles/traffic_*.json) were taken on.  A new layer is one more row (DESIGN.md "The host-side seam").
LAYERS = {
    "mpcg_fleet.h": {"sources": {"mpcg_fleet.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_fleet.h"]},
    "mpcg_path.h": {"sources": {"mpcg_path.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_path.h"]},
    "mpcg_guidance.h": {"sources": {"mpcg_guidance.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_guidance.h"]},
    "mpcg_active.h": {"sources": {"mpcg_active.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_active.h"]},
    "mpcg_road.h": {"sources": {"mpcg_road.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_road.h"]},
}
# the layers added after tests/test_layer_abi.py pinned the keys of LAYERS (decomp halfspaces): the same form,
# taken in by lib_sources() and build_lib alike; tests/test_layer_abi_later.py holds them to the same comparison.
# A change that may edit the pinned test folds the two tables together.
LATER_LAYERS = {
    "mpcg_decomp.h": {"sources": {"mpcg_decomp.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_decomp.h"]},
}
# the layers added after tests/test_layer_abi_later.py pinned the keys of LATER_LAYERS in turn (the SH-MPC scenario
# sampler, then the tracked-object layer): the same form once more.  tests/test_layer_abi_open.py checks every entry it finds here and pins no key
# set, so the next layer is one more row of this table; all_layers() stays the two pinned tables.
OPEN_LAYERS = {
    "mpcg_scenario.h": {"sources": {"mpcg_scenario.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_scenario.h"]},
    "mpcg_tracks.h": {"sources": {"mpcg_tracks.hip": ["-ffp-contract=off"]}, "headers": ["mpcg_tracks.h"]},
}
# csrc headers more than one layer includes: the entry points' checks and error text, the path evaluation,
# the wave arg-min
LAYER_SHARED_HEADERS = ["mpcg_host.h", "mpcg_spline.h", "mpcg_wave.h"]
HOST_SOURCES = ["host/mpcg_yaml.cpp", "host/mpcg_solver.cpp"]
HOST_HEADERS = ["mpc_planner_solver/mpcg_yaml.h", "mpc_planner_solver/mpcg_config.h", "mpc_planner_solver/state.h",
                "mpc_planner_solver/mpcg_solver_interface.h", "mpc_planner_solver/solver_interface.h"]
BUILD = os.path.join(PKG, "build")


def source_hash() -> str:
    """sha256 over the HIP kernel sources, the C ABI header and the build flags: the identity of
    the kernels a PMC profile was taken on (bench.py drops counters of other sources)."""
    import hashlib

    h = hashlib.sha256()
    for f in sorted(list(SOURCES) + HEADERS):
        h.update(f.encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(INCLUDE, "mpcg.h"), "rb") as fh:
        h.update(fh.read())
    h.update(repr((ARCH, sorted(SOURCES.items()))).encode())
    return h.hexdigest()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def lib_sources() -> dict:
    """every translation unit of libmpcg.so -> its extra flags: SOURCES, then the layers'"""
    srcs = dict(SOURCES)
    for layer in linked_layers().values():
        srcs.update(layer["sources"])
    return srcs


def all_layers() -> dict:
    """LAYERS, then LATER_LAYERS"""
    return {**LAYERS, **LATER_LAYERS}


def linked_layers() -> dict:
    """every layer linked into libmpcg.so: all_layers(), then OPEN_LAYERS"""
    return {**all_layers(), **OPEN_LAYERS}


def build_lib(force: bool = False, verbose: bool = False, extra_flags=(), out: str = LIB, sources=None) -> str:
    """libmpcg.so (or a diagnostic / variant build of it with extra_flags at `out`; `sources`
    restricts the built-in instance files of such a build)"""
    srcs = {k: v for k, v in lib_sources().items() if sources is None or k not in SOURCES or k in sources}
    layer_headers = LAYER_SHARED_HEADERS + [h for layer in linked_layers().values() for h in layer["headers"]]
    deps = [os.path.join(CSRC, f) for f in list(lib_sources()) + HEADERS + layer_headers] + \
        [os.path.join(INCLUDE, h) for h in ["mpcg.h"] + list(linked_layers())] + [__file__]
    if not force and not _stale(out, deps):
        return out
    objdir = os.path.join(BUILD, "obj" + ("_" + "_".join(f.strip("-").replace("=", "") for f in extra_flags)
                                          if extra_flags else ""))
    os.makedirs(objdir, exist_ok=True)
    common = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}"]
    objs, procs = [], []
    for src, flags in srcs.items():
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = common + list(flags) + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd))
        objs.append(obj)
    for p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, "hipcc")
    cmd = ["hipcc", f"--offload-arch={ARCH}", "-shared", "-fPIC", "-Wl,-soname,libmpcg.so", "-o", out + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(out + ".tmp", out)
    return out


def _hipcc_obj(src, obj, extra=()):
    cmd = ["hipcc", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}",
           *extra, "-c", src, "-o", obj]
    subprocess.run(cmd, check=True)
    return obj


def build_instance(layout, out_dir: str, force: bool = False) -> str:
    """libmpcg_inst_<name>.so: the kernel instance of `layout`'s dimensions (codegen
    mpcg_instance.hip) as a library that registers itself with libmpcg.so on load
    (native.load_instances)."""
    from . import codegen

    lib_mpcg = build_lib()
    os.makedirs(out_dir, exist_ok=True)
    src = os.path.join(out_dir, "mpcg_instance.hip")
    text = codegen.instance_source(layout)
    if not os.path.exists(src) or open(src).read() != text:
        with open(src, "w") as fh:
            fh.write(text)
    so = os.path.join(out_dir, f"libmpcg_inst_{layout.name}.so")
    deps = [src, lib_mpcg, os.path.join(INCLUDE, "mpcg.h")] + [os.path.join(CSRC, h) for h in HEADERS]
    if force or _stale(so, deps):
        obj = _hipcc_obj(src, os.path.join(out_dir, "mpcg_instance.o"))
        subprocess.run(["hipcc", f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", so + ".tmp", obj, f"-L{PKG}",
                        "-lmpcg", f"-Wl,-rpath,{PKG}"], check=True)
        os.replace(so + ".tmp", so)
    return so


def _build_probe(name: str, headers, force: bool) -> str:
    """build/probe/lib<name>.so from the test-only translation unit tests/cpp/<name>.hip, which includes
    `headers` of csrc; compiled with the flags of the kernel instances"""
    src = os.path.join(ROOT, "tests", "cpp", name + ".hip")
    out_dir = os.path.join(BUILD, "probe")
    so = os.path.join(out_dir, f"lib{name}.so")
    deps = [src, os.path.join(INCLUDE, "mpcg.h"), __file__] + [os.path.join(CSRC, h) for h in headers]
    if force or _stale(so, deps):
        os.makedirs(out_dir, exist_ok=True)
        obj = _hipcc_obj(src, os.path.join(out_dir, name + ".o"))
        subprocess.run(["hipcc", f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", so + ".tmp", obj], check=True)
        os.replace(so + ".tmp", so)
    return so


def build_stage_probe(force: bool = False) -> str:
    """single-thread kernels around the per-stage device functions of mpcg_device.h / mpcg_bicycle.h
    (tests/test_gpu_stage_functions.py)"""
    return _build_probe("stage_probe", HEADERS, force)


def build_mirror_probe(force: bool = False) -> str:
    """one wavefront per workgroup around mirror / mirror_blocks_ok / mirror_stage of mpcg_device.h
    (tests/test_gpu_mirror_blocks.py)"""
    return _build_probe("mirror_probe", ["mpcg_device.h"], force)


def build_fac_rows_probe(force: bool = False) -> str:
    """one wavefront around erk_unicycle of mpcg_device.h, one (z, pi) per lane
    (tests/test_gpu_fac_rows_probe.py)"""
    return _build_probe("fac_rows_probe", ["mpcg_device.h"], force)


# the switch-off builds tests/test_gpu_fac_rows.py compares the production library with:
# name under build/ab/ -> flags.  Only the N <= 20 unicycle family is built in: the test's shapes.
FAC_AB = {"fac_rows0": ["-DMPCG_FAC_INVARIANT_ROWS=0"],
          "fac_off": ["-DMPCG_FAC_INVARIANT_ROWS=0", "-DMPCG_FAC_PIVOT_SELECT=0"]}


def build_fac_ab(name: str, force: bool = False) -> str:
    """build/ab/<name>/libmpcg.so: libmpcg.so with FAC_AB[name]'s switches, instances of
    mpcg_inst_tmpc20.hip only"""
    out = os.path.join(BUILD, "ab", name, "libmpcg.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return build_lib(force=force, extra_flags=FAC_AB[name], out=out,
                     sources=("mpcg_kernels.hip", "mpcg_prepare.hip", "mpcg_inst_tmpc20.hip"))


# the build without the level tickets that tests/test_gpu_tail_levels.py and the A/B runs compare the production
# library with: the parent kernels.  `tail_poison` is the diagnostic build behind the carry set
# (NaN in everything else at every SQP-RTI boundary); __graft_entry__.build() does not make it.
# tail_g1 .. tail_g3: 1, 2 and 3 SQP-RTI iterations per level ticket (tests/test_gpu_tail_groups.py
# holds each of them to tail_off bit for bit).  tail_fences0 is the hand-over of §3.12 (acquire-release fetch-adds
# under explicit fences, one iteration per ticket): the A/B partner of the fence pair, not made by build().
TAIL_GROUPS = (1, 2, 3)
TAIL_AB = {"tail_off": ["-DMPCG_TAIL_LEVELS=0"], "tail_poison": ["-DMPCG_LEVEL_POISON"],
           **{f"tail_g{g}": [f"-DMPCG_TAIL_GROUP={g}"] for g in TAIL_GROUPS},
           "tail_fences0": ["-DMPCG_TAIL_FENCE_PAIR=0", "-DMPCG_TAIL_GROUP=1"]}


def build_tail_ab(name: str = "tail_off", force: bool = False) -> str:
    """build/ab/<name>/libmpcg.so: libmpcg.so with TAIL_AB[name]'s switches, instances of mpcg_inst_tmpc20.hip only"""
    out = os.path.join(BUILD, "ab", name, "libmpcg.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return build_lib(force=force, extra_flags=TAIL_AB[name], out=out,
                     sources=("mpcg_kernels.hip", "mpcg_prepare.hip", "mpcg_inst_tmpc20.hip"))


# the linearisation that forms its iterate-independent work again at every SQP-RTI iteration:
# `hrow_off` is the build tests/test_gpu_hrow_cache.py compares the production library with; the others switch
# one piece on alone, or keep only M00, M01, M11 in the cache (A/B runs; build() does not make them).
_HROW_OFF = {"cache": "-DMPCG_HROW_CACHE=0", "psi": "-DMPCG_PSI_SHARED=0"}
HROW_AB = {"hrow_off": list(_HROW_OFF.values()),
           **{f"hrow_only_{k}": [f for j, f in _HROW_OFF.items() if j != k] for k in _HROW_OFF},
           "hrow_cache1": ["-DMPCG_HROW_CACHE=1"]}


def build_hrow_ab(name: str = "hrow_off", force: bool = False) -> str:
    """build/ab/<name>/libmpcg.so: libmpcg.so with HROW_AB[name]'s switches, instances of mpcg_inst_tmpc20.hip only"""
    out = os.path.join(BUILD, "ab", name, "libmpcg.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return build_lib(force=force, extra_flags=HROW_AB[name], out=out,
                     sources=("mpcg_kernels.hip", "mpcg_prepare.hip", "mpcg_inst_tmpc20.hip"))


def build_erk_psi_probe(force: bool = False) -> str:
    """one wavefront around erk_unicycle of mpcg_device.h with and without sin / cos of psi given by the caller,
    one (z, pi) per lane (tests/test_gpu_erk_psi_probe.py)"""
    return _build_probe("erk_psi_probe", ["mpcg_device.h"], force)


def build_cpp(config="C2", force: bool = False, verbose: bool = False) -> dict:
    """The drop-in C++ MPCPlanner::Solver for one generated solver
    (dimensions are compile-time, as in the reference): codegen into
    build/<name>/, then libmpc_planner_solver.so -- the host sources plus the
    generated kernel instance of these dimensions -- and the test program
    tests/cpp/test_solver.cpp, linked against libmpcg.so.  `config` is a
    config name or a Layout."""
    from . import codegen
    from .layouts import config_layout

    lay = config_layout(config) if isinstance(config, str) else config
    lib_mpcg = build_lib()
    out = os.path.join(BUILD, lay.name)
    codegen.generate(lay, out)
    so = os.path.join(out, "libmpc_planner_solver.so")
    exe = os.path.join(out, "test_solver")
    srcs = [os.path.join(CSRC, s) for s in HOST_SOURCES] + [os.path.join(out, "mpc_planner_parameters.cpp")]
    inst = os.path.join(out, "mpcg_instance.hip")
    deps = srcs + [inst] + [os.path.join(INCLUDE, h) for h in HOST_HEADERS] + \
        [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(INCLUDE, "mpcg.h"), lib_mpcg, __file__]
    inc = [f"-I{os.path.join(out, 'include')}", f"-I{INCLUDE}"]
    if force or _stale(so, deps):
        objs = []
        for src in srcs:
            obj = os.path.join(out, os.path.basename(src).replace(".cpp", ".o"))
            cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-Wall", "-Wextra"] + inc + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
            objs.append(obj)
        objs.append(_hipcc_obj(inst, os.path.join(out, "mpcg_instance.o")))
        cmd = ["hipcc", f"--offload-arch={ARCH}", "-shared", "-fPIC"] + objs + \
              ["-o", so + ".tmp", f"-L{PKG}", "-lmpcg", f"-Wl,-rpath,{PKG}"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        os.replace(so + ".tmp", so)
    test_src = os.path.join(ROOT, "tests", "cpp", "test_solver.cpp")
    if os.path.exists(test_src) and (force or _stale(exe, [test_src, so])):
        cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra"] + inc + [test_src, "-o", exe, f"-L{out}",
                                                                      "-lmpc_planner_solver", f"-L{PKG}", "-lmpcg",
                                                                      f"-Wl,-rpath,{out}:{PKG}"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return {"dir": out, "lib": so, "test": exe}


if __name__ == "__main__":
    print(build_lib(force=True, verbose=True))
    print(build_cpp("C2", force=True, verbose=True))
