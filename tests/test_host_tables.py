"""The flush kernels' tile tables and the flush plan on a CPU (csrc/ekf_tables.h, csrc/ekf_flush_plan.h):
tests/cpp/tables_driver.cpp, a stand-alone program built with AddressSanitizer and
UndefinedBehaviorSanitizer, no GPU and no library.

For nb (tile rows of the landmark block) in 1-9, 16, 17, 64 and the capacity limit 2048, and every
rank of worlds of 1, 2, 3, 5 and 8 with a non-empty range, it checks that every stored tile is valid
in exactly one entry of each wave table and under exactly one 2 × 4 code, that every slot of every
entry names a tile of the block and every packed row block a row of it, that an entry's (row, column)
word matches its position, that the partition's ranges are contiguous with even boundaries, and that
the ranks' tables are disjoint and together the whole table. Two fixtures recorded from the loops,
the kernel-name function and the launcher conditions these headers replaced must be reproduced
exactly: tests/golden/flush_tables.txt (a 64-bit FNV-1a checksum per table, nb, world and rank) and
tests/golden/flush_kernel_names.txt (the kernel launched per precision, arithmetic, form, steps,
partitioned flag and kmax)."""
import os
import subprocess

from tests.test_sanitizers import ENV, ROOT, SAN


def test_tables_and_flush_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "tables_asan"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "tables_driver.cpp"), "-o", str(exe)], check=True)
    golden = os.path.join(ROOT, "tests", "golden")
    out = subprocess.run([str(exe), os.path.join(golden, "flush_tables.txt"),
                          os.path.join(golden, "flush_kernel_names.txt")], capture_output=True, text=True,
                         env=ENV, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
    assert "tables and flush plan: ok" in out.stdout
