// id_derivatives_facade_test.cpp -- ClusterTreeModel<double>::inverseDynamicsDerivativesBatch, both overloads, against the C ABI.
//
//   id_derivatives_facade_test <urdf>
// B states of the model: the host-array overload, the device-array overload on a stream, and grbda_rnea_derivatives_f64 on the model's
// own plan must give the same bits in all three matrices (they are one code path); the matrices are also held to what they mean on the
// host: dtau_dydd is symmetric, and tau(ydd + e_j) - tau(ydd) through inverseDynamicsBatch is its column j to 1e-9 of 1 + max |H|.
// Built with g++ (the HIP runtime API only: allocation and copies, no device code in this file).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "grbda/Dynamics/ClusterTreeModel.h"

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

using namespace grbda;

static bool same_bits(const std::vector<double> &a, const std::vector<double> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: id_derivatives_facade_test <urdf>\n");
        return 2;
    }
    ClusterTreeModel<double> m{std::string(argv[1])};
    const size_t B = 7, nq = m.getNumPositions(), nv = m.getNumDegreesOfFreedom(), nn = nv * nv;
    std::vector<double> q(B * nq), qd(B * nv), ydd(B * nv);
    unsigned long long sd = 0x9E3779B97F4A7C15ull;
    auto uni = [&]() { sd = sd * 6364136223846793005ull + 1442695040888963407ull; return (double)(sd >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    for (size_t s = 0; s < B; s++) {
        for (size_t j = 0; j < nq; j++) q[s * nq + j] = uni();
        if (nq == nv + 1) {  // floating base: a unit quaternion in the last four of its seven positions
            double nrm = 0;
            for (int j = 3; j < 7; j++) nrm += q[s * nq + j] * q[s * nq + j];
            for (int j = 3; j < 7; j++) q[s * nq + j] /= std::sqrt(nrm);
        }
        for (size_t j = 0; j < nv; j++) { qd[s * nv + j] = uni(); ydd[s * nv + j] = uni(); }
    }
    // host-array overload
    std::vector<double> h_dq(B * nn), h_dqd(B * nn), h_H(B * nn);
    m.inverseDynamicsDerivativesBatch(q.data(), qd.data(), ydd.data(), h_dq.data(), h_dqd.data(), h_H.data(), B);

    // device-array overload and the C ABI, on one stream
    hipStream_t stream = nullptr;
    if (hipSetDevice(0) != hipSuccess || hipStreamCreate(&stream) != hipSuccess) return 1;
    double *dq_ = nullptr, *dqd_ = nullptr, *dydd_ = nullptr, *out[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (hipMalloc((void **)&dq_, B * nq * sizeof(double)) != hipSuccess || hipMalloc((void **)&dqd_, B * nv * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&dydd_, B * nv * sizeof(double)) != hipSuccess)
        return 1;
    for (double *&o : out)
        if (hipMalloc((void **)&o, B * nn * sizeof(double)) != hipSuccess) return 1;
    (void)hipMemcpy(dq_, q.data(), B * nq * sizeof(double), hipMemcpyHostToDevice);
    (void)hipMemcpy(dqd_, qd.data(), B * nv * sizeof(double), hipMemcpyHostToDevice);
    (void)hipMemcpy(dydd_, ydd.data(), B * nv * sizeof(double), hipMemcpyHostToDevice);
    m.inverseDynamicsDerivativesBatch(dq_, dqd_, dydd_, out[0], out[1], out[2], B, 0, stream);
    const int rc_abi = grbda_rnea_derivatives_f64(m.plan(), dq_, dqd_, dydd_, 1e-6, out[3], out[4], out[5], B, 0, stream);
    if (rc_abi != GRBDA_OK || hipStreamSynchronize(stream) != hipSuccess) {
        std::fprintf(stderr, "grbda_rnea_derivatives_f64: %d %s\n", rc_abi, grbda_last_error());
        return 1;
    }
    std::vector<std::vector<double>> got(6, std::vector<double>(B * nn));
    for (int i = 0; i < 6; i++) (void)hipMemcpy(got[i].data(), out[i], B * nn * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(dq_); (void)hipFree(dqd_); (void)hipFree(dydd_);
    for (double *o : out) (void)hipFree(o);
    (void)hipStreamDestroy(stream);

    int bad = 0;
    const std::vector<double> *host[3] = {&h_dq, &h_dqd, &h_H};
    const char *names[3] = {"dtau_dq", "dtau_dqd", "dtau_dydd"};
    for (int k = 0; k < 3; k++) {
        const bool dev_eq = same_bits(got[k], got[3 + k]), host_eq = same_bits(got[k], *host[k]);
        std::printf("  %-9s device overload == C ABI: %d, == host overload: %d\n", names[k], (int)dev_eq, (int)host_eq);
        bad |= !dev_eq || !host_eq;
    }
    // what the matrices mean: H symmetric, and its columns are the unit-acceleration differences of the inverse dynamics
    double scale = 0, asym = 0, col_err = 0, dq_max = 0, dqd_max = 0;
    for (size_t i = 0; i < B * nn; i++) {
        scale = std::max(scale, std::fabs(h_H[i]));
        dq_max = std::max(dq_max, std::fabs(h_dq[i]));
        dqd_max = std::max(dqd_max, std::fabs(h_dqd[i]));
        if (!std::isfinite(h_H[i]) || !std::isfinite(h_dq[i]) || !std::isfinite(h_dqd[i])) bad = 1;
    }
    std::vector<double> tau0(B * nv), tau1(B * nv), y1;
    m.inverseDynamicsBatch(q.data(), qd.data(), ydd.data(), tau0.data(), B);
    for (size_t j = 0; j < nv; j++) {
        y1 = ydd;
        for (size_t s = 0; s < B; s++) y1[s * nv + j] += 1.0;
        m.inverseDynamicsBatch(q.data(), qd.data(), y1.data(), tau1.data(), B);
        for (size_t s = 0; s < B; s++)
            for (size_t i = 0; i < nv; i++) {
                col_err = std::max(col_err, std::fabs(tau1[s * nv + i] - tau0[s * nv + i] - h_H[s * nn + i * nv + j]));
                asym = std::max(asym, std::fabs(h_H[s * nn + i * nv + j] - h_H[s * nn + j * nv + i]));
            }
    }
    std::printf("  max |H| %.3g, |H - H^T| %.3g, columns of H against unit differences of ID %.3g; max |dq| %.3g, |dqd| %.3g\n", scale, asym,
                col_err, dq_max, dqd_max);
    bad |= !(col_err < 1e-9 * (1.0 + scale)) || !(asym < 1e-12 * (1.0 + scale)) || !(dq_max > 0) || !(dqd_max > 0);
    std::printf(bad ? "FAILED\n" : "OK\n");
    return bad;
}
