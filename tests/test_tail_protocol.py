"""The level-ticket protocol of csrc/mpcg_tail.h under host threads (tests/cpp/tail_protocol.cpp): the
stand-alone program is built plain and with ThreadSanitizer and run as an ordinary program.  It exits
non-zero when a (solve, level) ran twice, out of order or not at all, when a level read a carry its
predecessor did not write, when a boundary word was touched more than twice, or when the atomic operations
counted inside the atomic differ from one per level ticket past level 0 plus one per level that goes on (a retry
or a spin); under ThreadSanitizer any access to a solve's
plain carry that the boundary word does not order is a reported race (exit code 66)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tail_protocol.cpp")
INC = os.path.join(ROOT, "oscar_mpc_planner_mr_modification_amd", "csrc")
# threads, solves, levels, K, seed: every solve by levels, a whole-solve head, K below the thread count's reach,
# none by levels, and the 16 levels the words hold
CASES = [(8, 300, 10, 300, 1), (16, 300, 10, 263, 2), (4, 300, 10, 100, 3), (12, 200, 10, 0, 4), (16, 150, 16, 150, 5),
         (5, 400, 2, 400, 6)]


def _build(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, f"-I{INC}", SRC, "-o", exe,
                    "-pthread"], check=True)
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=thread",)], ids=["plain", "tsan"])
def test_protocol_under_host_threads(tmp_path, flags):
    exe = _build(tmp_path, "tail_protocol", flags)
    env = dict(os.environ, TSAN_OPTIONS="exitcode=66 halt_on_error=1")
    for case in CASES:
        p = subprocess.run([exe, *map(str, case)], capture_output=True, text=True, timeout=120, env=env)
        assert p.returncode == 0, (case, p.returncode, p.stdout[-500:], p.stderr[-2000:])
        assert "errors 0" in p.stdout, p.stdout


def test_ticket_numbering(tmp_path):
    """decode() against the numbering of the header's comment, through a tiny program"""
    src = tmp_path / "decode.cpp"
    src.write_text('#include <cstdio>\n#include "mpcg_tail.h"\nint main() {\n'
                   '  const mpcg::tail::Plan p{10, 4, 3};\n'
                   '  for (unsigned t = 0; t < 20; ++t) { auto k = mpcg::tail::decode(p, t);'
                   ' std::printf("%d:%d:%d ", k.kind, k.sol, k.lvl); }\n'
                   '  auto e = mpcg::tail::decode(p, 0xFFFFFFF0u); std::printf("%d", e.kind);\n'
                   '  std::printf(" %d %d %d %d", mpcg::tail::plan_k(10, 10, 3, 4), mpcg::tail::plan_k(10, 4, 17, 4),'
                   ' mpcg::tail::plan_k(10, 4, 3, 40), mpcg::tail::plan_k(10, 4, 3, 0));\n}\n')
    exe = str(tmp_path / "decode")
    subprocess.run([shutil.which("g++") or "c++", "-std=c++17", f"-I{INC}", str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    whole = [f"0:{t}:0" for t in range(6)]                                    # D = 6 whole solves
    levels = [f"1:{6 + j}:{lv}" for lv in range(3) for j in range(4)]         # level-major over the last 4
    assert out[:18] == whole + levels
    assert out[18:20] == ["2:10:0", "2:10:0"] and out[20] == "2"             # past D + L K: the wave leaves
    assert out[21:] == ["0", "0", "10", "0"]   # fits the grid / too many levels / clamped to the batch / none asked
