// frame_jacobians_facade_test.cpp -- ClusterTreeModel::frameJacobiansBatch of the facade.  Host side: the refusals that are decided before a
// device is looked for.  With a device present the batch call runs three states, two frames and both axes, and is held to the device entry
// point grbda_frame_jacobians_f64 on the same states (1e-12).
//   frame_jacobians_facade_test model.urdf
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "grbda/grbda.h"

using namespace grbda;

static int failures = 0;
static void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAIL %s\n", what);
        failures++;
    }
}
template <class Call>
static std::string refused(Call call)
{
    try {
        call();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return "";
}
template <class T>
static T *to_device(const std::vector<T> &h)
{
    T *d = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d), h.size() * sizeof(T)) != hipSuccess) throw std::runtime_error("hipMalloc");
    if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy");
    return d;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    ClusterTreeModel<double> model;
    model.buildModelFromURDF(argv[1]);
    const size_t nq = model.getNumPositions(), nv = model.getNumDegreesOfFreedom(), B = 3;
    const int n = 2, last = static_cast<int>(model.bodies().size()) - 1;
    const int bodies[2] = {last, 0};
    const double offsets[6] = {0.03, -0.07, 0.11, -0.05, 0.02, -0.2};
    std::vector<double> q(B * nq), qd(B * nv), J(B * n * 6 * nv), drift(B * n * 6);
    for (size_t b = 0; b < B; b++) {
        for (size_t i = 0; i < nq; i++) q[b * nq + i] = 0.1 * std::sin(1.0 + 0.7 * i + 2.1 * b);
        for (size_t i = 0; i < nv; i++) qd[b * nv + i] = 0.5 * std::cos(0.3 + 1.3 * i + 0.9 * b);
        if (nq == nv + 1) {  // a floating base: a unit quaternion
            double *e = &q[b * nq + 3], s = 0;
            e[0] += 1.0;
            for (int i = 0; i < 4; i++) s += e[i] * e[i];
            for (int i = 0; i < 4; i++) e[i] /= std::sqrt(s);
        }
    }
    // decided on the host, device or not
    const auto call = [&](const double *q_, const double *qd_, int n_, const int *bodies_, double *J_, double *d_, size_t B_ = 3) {
        return refused([&] { model.frameJacobiansBatch(q_, qd_, n_, bodies_, offsets, false, J_, d_, B_); });
    };
    expect(call(nullptr, qd.data(), n, bodies, J.data(), drift.data()).find("null argument") != std::string::npos, "a null q is refused");
    expect(call(q.data(), qd.data(), 17, bodies, J.data(), drift.data()).find("0..16") != std::string::npos, "seventeen frames are refused");
    const int bad[2] = {last + 1, 0};
    expect(call(q.data(), qd.data(), n, bad, J.data(), drift.data()).find("body index") != std::string::npos, "a bad body index is refused");
    expect(call(q.data(), qd.data(), n, bodies, nullptr, nullptr).find("no output asked for") != std::string::npos, "no output is refused");
    expect(call(q.data(), nullptr, n, bodies, J.data(), drift.data()).find("needs qd") != std::string::npos, "the drift without qd is refused");
    expect(call(q.data(), qd.data(), n, bodies, J.data(), J.data()).find("overlap") != std::string::npos, "overlapping outputs are refused");
    expect(call(q.data(), qd.data(), n, bodies, J.data(), drift.data(), 0).empty(), "B == 0: nothing to do");
    expect(call(q.data(), nullptr, 0, nullptr, nullptr, nullptr).empty(), "n == 0: nothing to do");

    if (grbda_device_count() > 0) {
        double *dq = to_device(q), *dqd = to_device(qd), *dJ = to_device(J), *dd = to_device(drift);
        std::vector<double> J_dev(J.size()), d_dev(drift.size());
        for (int world = 0; world < 2; world++) {
            model.frameJacobiansBatch(q.data(), qd.data(), n, bodies, offsets, world != 0, J.data(), drift.data(), B);
            const int rc = grbda_frame_jacobians_f64(model.plan(), dq, dqd, n, bodies, offsets, world, dJ, dd, B, 0, nullptr);
            expect(rc == GRBDA_OK && hipDeviceSynchronize() == hipSuccess, "the device call runs");
            expect(hipMemcpy(J_dev.data(), dJ, J.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess, "J comes back");
            expect(hipMemcpy(d_dev.data(), dd, drift.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess, "the drift comes back");
            double worst = 0, top = 0;
            for (size_t i = 0; i < J.size(); i++) {
                worst = std::fmax(worst, std::fabs(J[i] - J_dev[i]));
                top = std::fmax(top, std::fabs(J[i]));
            }
            for (size_t i = 0; i < drift.size(); i++) worst = std::fmax(worst, std::fabs(drift[i] - d_dev[i]));
            expect(worst <= 1e-12 && top > 0.1, world ? "world frame: the facade is the device call" : "body frame: the facade is the device call");
            // J alone gives the same J
            std::vector<double> J_only(J.size());
            model.frameJacobiansBatch(q.data(), nullptr, n, bodies, offsets, world != 0, J_only.data(), nullptr, B);
            expect(J_only == J, "J alone is the same J");
        }
        (void)hipFree(dq);
        (void)hipFree(dqd);
        (void)hipFree(dJ);
        (void)hipFree(dd);
    } else {
        expect(call(q.data(), qd.data(), n, bodies, J.data(), drift.data()).find("no HIP device") != std::string::npos,
               "a valid call without a device says so");
    }
    if (failures == 0) std::printf("OK\n");
    return failures ? 1 : 0;
}
