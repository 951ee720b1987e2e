"""The kernel sources as build.py sees them (no GPU, no compiler): csrc/ holds one small .hip file per
compilation unit beside the device code they include by topic, the library's source hash covers every file,
and no unit is selected by number."""
import os

from slam_ros_amd import build

SUFFIXES = (".hip", ".h")


def _csrc_files():
    found = []
    for base, _dirs, files in os.walk(build.CSRC):
        found += [os.path.join(base, f) for f in files if f.endswith(SUFFIXES)]
    return sorted(found)


def test_every_source_is_hashed():
    deps = set(build.source_deps())
    files = _csrc_files()
    assert files, build.CSRC
    missing = [f for f in files if f not in deps]
    assert not missing, missing
    assert os.path.join(build.ROOT, "include", "slam_ekf.h") in deps
    assert os.path.abspath(build.__file__) in deps
    assert all(os.path.isfile(d) for d in deps)


def test_every_unit_exists():
    assert build.UNITS and len(build.UNITS) == len(set(build.UNITS))
    for u in build.UNITS:
        assert isinstance(u, str) and os.path.isfile(os.path.join(build.CSRC, u)), u


def test_no_unit_number_switch():
    for f in _csrc_files():
        with open(f, encoding="utf-8") as src:
            assert "EKF_TU" not in src.read(), f
