// integrate_facade_test.cpp -- ori::quatProduct, ori::integrateQuat (world-frame omega) and ori::integrateQuatImplicit (body-frame
// omega) of the facade against closed-form rotations.  Host only: no device is touched.
//   integrate_facade_test
#include <cmath>
#include <cstdio>

#include "grbda/grbda.h"

using namespace grbda;

static int failures = 0;
static void expect_near(const Quat<double> &a, const Quat<double> &b, double tol, const char *what)
{
    // a quaternion and its negative are the same rotation
    double d0 = 0, d1 = 0;
    for (int i = 0; i < 4; i++) {
        d0 = std::fmax(d0, std::fabs(a[i] - b[i]));
        d1 = std::fmax(d1, std::fabs(a[i] + b[i]));
    }
    const double d = std::fmin(d0, d1);
    if (!(d <= tol)) {
        std::printf("FAIL %s: %.3e > %.1e\n", what, d, tol);
        failures++;
    }
}

int main()
{
    const double tol = 1e-14, pi = 3.14159265358979323846;
    const Quat<double> one{1.0, 0.0, 0.0, 0.0};

    // a rotation about one axis by a known angle: omega = rate e_z for dt seconds from the identity -> (cos(a/2), 0, 0, sin(a/2))
    {
        const double rate = 0.7, dt = 0.3, a = rate * dt;
        const Quat<double> want{std::cos(a / 2), 0.0, 0.0, std::sin(a / 2)};
        expect_near(ori::integrateQuatImplicit(one, Vec3<double>{0.0, 0.0, rate}, dt), want, tol, "implicit, z axis from identity");
        expect_near(ori::integrateQuat(one, Vec3<double>{0.0, 0.0, rate}, dt), want, tol, "world, z axis from identity");
        // from a start that is itself a rotation about z the angles add, in both frames (the axis is the same in both)
        const Quat<double> start{std::cos(0.2), 0.0, 0.0, std::sin(0.2)}, sum{std::cos(0.2 + a / 2), 0.0, 0.0, std::sin(0.2 + a / 2)};
        expect_near(ori::integrateQuatImplicit(start, Vec3<double>{0.0, 0.0, rate}, dt), sum, tol, "implicit, angles add");
        expect_near(ori::integrateQuat(start, Vec3<double>{0.0, 0.0, rate}, dt), sum, tol, "world, angles add");
        // a quarter turn about x in one second
        const Quat<double> qx{std::cos(pi / 4), std::sin(pi / 4), 0.0, 0.0};
        expect_near(ori::integrateQuatImplicit(one, Vec3<double>{pi / 2, 0.0, 0.0}, 1.0), qx, tol, "implicit, quarter turn about x");
    }
    // zero omega: the orientation stays (and the (1,0,0) axis of the reference produces no NaN)
    {
        const Quat<double> start = ori::rpyToQuat(Vec3<double>{0.3, -0.5, 0.9});
        expect_near(ori::integrateQuatImplicit(start, Vec3<double>{0.0, 0.0, 0.0}, 0.1), start, tol, "implicit, zero omega");
        expect_near(ori::integrateQuat(start, Vec3<double>{0.0, 0.0, 0.0}, 0.1), start, tol, "world, zero omega");
    }
    // two half steps with a constant omega compose to the full step (rotations about one axis commute)
    {
        const Quat<double> start = ori::rpyToQuat(Vec3<double>{-0.4, 0.2, 0.6});
        const Vec3<double> w{0.3, -0.8, 0.5};
        const double dt = 0.25;
        expect_near(ori::integrateQuatImplicit(ori::integrateQuatImplicit(start, w, dt / 2), w, dt / 2), ori::integrateQuatImplicit(start, w, dt),
                    tol, "implicit, two half steps");
        expect_near(ori::integrateQuat(ori::integrateQuat(start, w, dt / 2), w, dt / 2), ori::integrateQuat(start, w, dt), tol,
                    "world, two half steps");
    }
    // a body-frame omega and the same omega rotated into world axes give the same quaternion from the two functions
    {
        const Quat<double> start = ori::rpyToQuat(Vec3<double>{0.7, -0.3, 0.4});
        const Vec3<double> wb{0.9, 0.4, -0.6};
        const Mat3<double> R = ori::quaternionToRotationMatrix(start);  // v_body = R v_world
        Vec3<double> ww;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) ww[i] += R(j, i) * wb[j];  // R^T omega_body
        expect_near(ori::integrateQuatImplicit(start, wb, 0.2), ori::integrateQuat(start, ww, 0.2), tol, "body and world frame agree");
    }
    // the product itself: i j = k, and the norm is multiplicative
    {
        const Quat<double> i{0.0, 1.0, 0.0, 0.0}, j{0.0, 0.0, 1.0, 0.0}, k{0.0, 0.0, 0.0, 1.0};
        const Quat<double> ij = ori::quatProduct(i, j);
        double d = 0;
        for (int a = 0; a < 4; a++) d = std::fmax(d, std::fabs(ij[a] - k[a]));
        if (d != 0.0) {
            std::printf("FAIL i j = k\n");
            failures++;
        }
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
