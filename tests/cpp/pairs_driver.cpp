// Includes slam_ekf.h as C++ and checks what ekf_gate_landmarks promises without a context: the record's
// size and field offsets, the status bits, and EKF_EINVAL for a NULL context from both forms (no GPU).
//
// usage: pairs_driver            the NULL-context returns: "null <rc> <rc>"
//        pairs_driver --sizeof   sizeof(ekf_pair_hit) and its field offsets
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "slam_ekf.h"

static_assert(sizeof(ekf_pair_hit) == 72, "ekf_pair_hit is 72 bytes");
static_assert(EKF_PH_FLIP_NEAREST == 1 && EKF_PH_FLIP_FIRST == 2 && EKF_PH_SINGULAR == 4, "ekf_pair_hit.status bits");

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--sizeof")) {
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ekf_pair_hit), offsetof(ekf_pair_hit, nearest),
                    offsetof(ekf_pair_hit, first), offsetof(ekf_pair_hit, npass), offsetof(ekf_pair_hit, status),
                    offsetof(ekf_pair_hit, d2_nearest), offsetof(ekf_pair_hit, d2_first), offsetof(ekf_pair_hit, C),
                    offsetof(ekf_pair_hit, delta));
        return 0;
    }
    ekf_pair_hit hits[2];
    double d2[4];
    const int host = ekf_gate_landmarks(nullptr, 0, 0.4, hits, d2);
    const int dev = ekf_gate_landmarks_device(nullptr, 0.4, hits, nullptr);
    std::printf("null %d %d\n", host, dev);
    return host == EKF_EINVAL && dev == EKF_EINVAL ? 0 : 1;
}
