// centroidal_facade_test.cpp -- ClusterTreeModel::totalMass, energyBatch and centroidalBatch of the facade.  Host side: the total mass of
// a model read from a URDF against the sum of its bodies' masses, and the refusals that are decided before a device is looked for.  With
// a device present the batch calls also run one state and are checked against each other (P = M c_dot, PE = -M g . c).
//   centroidal_facade_test model.urdf
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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    ClusterTreeModel<double> model;
    model.buildModelFromURDF(argv[1]);
    double sum = 0;
    for (const auto &body : model.bodies()) sum += body.inertia_.getMatrix()(3, 3);
    const double M = model.totalMass();
    expect(M > 0 && std::fabs(M - sum) <= 1e-12 * sum, "totalMass is the sum of the body masses");

    const size_t nq = model.getNumPositions(), nv = model.getNumDegreesOfFreedom();
    std::vector<double> q(nq, 0.0), qd(nv, 0.1), ydd(nv, 0.0), ke(1), pe(1), com(3), cv(3), h(6), hd(6);
    if (nq == nv + 1) q[3] = 1.0;  // the identity quaternion of a floating base
    // decided on the host, device or not
    expect(refused([&] { model.energyBatch(q.data(), qd.data(), nullptr, nullptr, 1); }).find("no output asked for") != std::string::npos,
           "energyBatch without outputs is refused");
    expect(refused([&] { model.energyBatch(q.data(), nullptr, ke.data(), pe.data(), 1); }).find("need qd") != std::string::npos,
           "kinetic without qd is refused");
    expect(refused([&] { model.centroidalBatch(q.data(), qd.data(), nullptr, com.data(), cv.data(), h.data(), hd.data(), 1); }).find("hdot needs ydd") !=
               std::string::npos,
           "hdot without ydd is refused");
    expect(refused([&] { model.centroidalBatch(q.data(), qd.data(), ydd.data(), com.data(), com.data(), nullptr, nullptr, 1); }).find("overlap") !=
               std::string::npos,
           "overlapping outputs are refused");
    model.energyBatch(q.data(), nullptr, nullptr, pe.data(), 0);  // B == 0: nothing to do

    if (grbda_device_count() > 0) {
        model.energyBatch(q.data(), qd.data(), ke.data(), pe.data(), 1);
        model.centroidalBatch(q.data(), qd.data(), ydd.data(), com.data(), cv.data(), h.data(), hd.data(), 1);
        const SVec<double> g6 = model.getGravity();
        double pe_ref = 0;
        for (int i = 0; i < 3; i++) {
            pe_ref -= M * g6[3 + i] * com[i];
            expect(std::fabs(h[3 + i] - M * cv[i]) <= 1e-10 * (1 + std::fabs(h[3 + i])), "linear momentum is M c_dot");
        }
        expect(ke[0] > 0 && std::fabs(pe[0] - pe_ref) <= 1e-10 * (1 + std::fabs(pe_ref)), "kinetic > 0 and potential is -M g . c");
    } else {
        expect(refused([&] { model.energyBatch(q.data(), qd.data(), ke.data(), pe.data(), 1); }).find("no HIP device") != std::string::npos,
               "a valid call without a device says so");
    }
    if (failures == 0) std::printf("OK\n");
    return failures ? 1 : 0;
}
