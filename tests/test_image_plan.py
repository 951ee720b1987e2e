"""The instance image's tables on a CPU (csrc/ekf_image_plan.h): tests/cpp/image_driver.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer, no GPU and no library.

Over the grid of tests/test_resample_plan.py (nb in {1, 3, 5, 64}, E in {1, 4, 8}, element sizes 2, 4
and 8, 0 / 1 / T − 1 / 2T − 1 pending ring slots, also wrapping round the ring, one and two live
landmark buffers at either parity, stored and symmetric U rows, each plane mode) it checks that the
sections are 16-byte aligned and the image has the closed-form size, that the export table covers every
image byte exactly once (sections by copies, padding by zeros), that export of instance s followed by
import into slot d of the same layout is the byte map of resample_plan with src[d] = s, that a
destination at another ring position and buffer parity receives the sections by their meaning, that
the completion words and only they are re-tag pieces, and that the key follows every keyed field and
not E."""
import os
import subprocess

from tests.test_sanitizers import ENV, ROOT, SAN


def test_image_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "image_asan"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "image_driver.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
    assert "image plan: ok" in out.stdout
