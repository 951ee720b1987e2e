"""ekf_resample's copy table on a CPU (csrc/ekf_resample_plan.h): tests/cpp/resample_driver.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, no GPU and no library.

Over nb in {1, 3, 5, 64}, E in {1, 4, 8}, element sizes 2, 4 and 8, 0 / 1 / T − 1 / 2T − 1 pending ring
slots (also wrapping round the ring), one and two live landmark buffers, stored and symmetric U rows,
each plane mode and source lists with and without duplicated sources, it checks that the table covers
every destination byte exactly once, reads nothing it writes, reads for instance e only instance
src[e]'s slices at the same offsets, keeps the alignment classes, moves the closed-form number of
bytes and is empty for the identity list."""
import os
import subprocess

from tests.test_sanitizers import ENV, ROOT, SAN


def test_resample_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "resample_asan"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "resample_driver.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
    assert "resample plan: ok" in out.stdout
