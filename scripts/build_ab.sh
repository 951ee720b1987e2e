# A/B timing builds: bash scripts/build_ab.sh NAME CSRC_FILE PATCHED → slam_ros_amd/lib/xp_NAME.so
# (this tree's csrc/ with PATCHED in place of its CSRC_FILE, e.g. ekf_kernels.hip; the library's
# compilation units in parallel; selected at run time by SLAM_EKF_LIB)
set -e
[ $# -eq 3 ] || { echo "usage: bash scripts/build_ab.sh NAME CSRC_FILE PATCHED" >&2; exit 2; }
cd "$(dirname "$0")/.."
[ -f "slam_ros_amd/csrc/$2" ] || { echo "no slam_ros_amd/csrc/$2" >&2; exit 1; }
T=$(mktemp -d)
mkdir -p $T/include $T/p/csrc
cp include/slam_ekf.h $T/include/
cp slam_ros_amd/csrc/*.h slam_ros_amd/csrc/*.hip $T/p/csrc/
cp "$3" "$T/p/csrc/$2"
python3 -c "import sys; sys.path.insert(0, '.'); from slam_ros_amd import build as b; b.build_variant('slam_ros_amd/lib/xp_$1.so', [], csrc='$T/p/csrc')"
rm -rf $T
