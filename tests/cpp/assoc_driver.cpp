// Drives BasicRobot::associateJoint (slam_ros_amd/host/robot_ekf.hpp): the two scans of gate_driver.cpp
// build and re-observe a small map; then the five observations as a third pose would see them are
// associated jointly, each line offered its own landmark and its right-hand neighbour's (the second one
// last), under a loose bound, with that pose's encoder reading, the state untouched. The `line` / message
// types are the test doubles of dropin_driver.cpp.
//
// usage: assoc_driver            the hit
//        assoc_driver --sizeof   sizeof(ekf_assoc_hit) and its field offsets (no GPU)
// stdout: "hit m status d2 logdet", "assign a0 .. a4", then "saved s"; exit 3 if the GPU path fails.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "robot_ekf.hpp"

struct Mat2 {
    size_t size1 = 2, size2 = 2, tda = 2;
    double data[4] = {0, 0, 0, 0};
};
struct polar_point {
    polar_point(double a = 0, double rr = 0) : alfa(a), r(rr) {}
    double alfa, r;
};
struct line {
    double alfa = 0, r = 0;
    Mat2* C_AR = nullptr;
    std::vector<polar_point> lineInterval;
};
struct Float32MultiArray {
    std::vector<float> data;
};
typedef slam_ekf::BasicRobot<line, Float32MultiArray, 100> Rover;

int main(int argc, char** argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "--sizeof")) {
        std::printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(ekf_assoc_hit), offsetof(ekf_assoc_hit, m),
                    offsetof(ekf_assoc_hit, status), offsetof(ekf_assoc_hit, nodes), offsetof(ekf_assoc_hit, reserved),
                    offsetof(ekf_assoc_hit, d2), offsetof(ekf_assoc_hit, logdet), offsetof(ekf_assoc_hit, assign));
        return 0;
    }
    static const double obs[5][2] = {{-2.4, 1.1}, {-1.0, 2.3}, {0.2, 0.8}, {1.3, 3.1}, {2.6, 1.9}};
    try {
        Rover* rp = new Rover(0, 0, 0);
        Rover& rover = *rp;
        for (int k = 0; k < 2; k++) {
            const double enc[3] = {0.01 * (k + 1), -0.005 * (k + 1), 0.002 * (k + 1)};
            std::vector<Mat2> covs(5);
            std::vector<line> lines(5);
            for (int i = 0; i < 5; i++) {
                lines[i].alfa = obs[i][0] - (k ? enc[2] : 0.0);
                lines[i].r = obs[i][1];
                covs[i].data[0] = covs[i].data[3] = 1e-2;
                lines[i].C_AR = &covs[i];
            }
            rover.localize(lines, nullptr, enc);
        }
        const double enc[3] = {0.022, -0.011, 0.0044};
        std::vector<Mat2> covs(5);
        std::vector<line> lines(5);
        for (int i = 0; i < 5; i++) {
            lines[i].alfa = obs[i][0] - enc[2];
            lines[i].r = obs[i][1];
            covs[i].data[0] = covs[i].data[3] = 1e-2;
            lines[i].C_AR = &covs[i];
        }
        std::vector<int32_t> cand;
        for (int i = 0; i < 5; i++) {
            cand.push_back((i + 1) % 5);
            cand.push_back(i);
        }
        const std::vector<double> bound = {0.0, 9.0, 13.0, 17.0, 20.0, 23.0};
        ekf_assoc_hit hit;
        if (!rover.associateJoint(lines, cand, bound, hit, enc)) return 3;
        std::printf("hit %d %d %.17g %.17g\n", hit.m, hit.status, hit.d2, hit.logdet);
        std::printf("assign %d %d %d %d %d\n", hit.assign[0], hit.assign[1], hit.assign[2], hit.assign[3], hit.assign[4]);
        int saved = 0;
        if (!rover.downloadP(nullptr, &saved)) return 3;
        std::printf("saved %d\n", saved);
        delete rp;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
