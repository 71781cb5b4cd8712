// test_batch_overlap.cpp — BatchedSimulator::overlapMatrix, kernelMatrix and overlapsWith of the
// C++17 layer against the header-only CPU oracle (oracle/cpu_simulator.hpp) run once per trajectory
// with that trajectory's angles written into the circuit, and the exception types.  The bound is
// the project's 1e-12 per component (the members come from a run; the summation's own bound
// 2 * 2^(n+1) * 2^-53 is 4.5e-13 at n = 10).
#include <qsim/Circuit.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <random>
#include <stdexcept>
#include <vector>

#include "cpu_simulator.hpp"
#include "harness.hpp"

using cplx = std::complex<double>;
static const int P = 7;

// Every parameterised type, both control orders; any n >= 3.
static qsim::Circuit ansatz(int n, const std::vector<double>& a) {
    qsim::Circuit c(n);
    for (int q = 0; q < n; ++q) c.h(q);
    c.rx(0, a[0]).ry(n - 1, a[1]).rz(n / 2, a[2]);
    for (int q = 0; q + 1 < n; ++q) c.cnot(q, q + 1);
    c.cry(1, n - 2, a[3]).crz(n - 1, 2, a[4]).t(1).toffoli(0, 1, n - 1);
    c.ry(n / 2, a[5]).rz(0, a[6]).swap(2, n - 1);
    return c;
}

static std::vector<double> random_angles(int B, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> dist(-3.0, 3.0);
    std::vector<double> angles((size_t)B * P);
    for (double& v : angles) v = dist(rng);
    return angles;
}

static std::vector<std::vector<cplx>> oracle_states(int n, int B, const std::vector<double>& angles) {
    std::vector<std::vector<cplx>> out;
    for (int t = 0; t < B; ++t) {
        qsim_oracle::CPUSimulator cpu(n);
        cpu.run(ansatz(n, std::vector<double>(angles.begin() + t * P, angles.begin() + (t + 1) * P)));
        out.push_back(cpu.getStateVector());
    }
    return out;
}

static cplx vdot(const std::vector<cplx>& a, const std::vector<cplx>& b) {
    cplx acc = 0.0;
    for (size_t i = 0; i < a.size(); ++i) acc += std::conj(a[i]) * b[i];
    return acc;
}

static double component_error(cplx got, cplx want) {
    return std::max(std::fabs(got.real() - want.real()), std::fabs(got.imag() - want.imag()));
}

static void check_shape(int n, int B, int B2) {
    const std::vector<double> angles = random_angles(B, 11u + (unsigned)n), angles2 = random_angles(B2, 5u);
    qsim::BatchedSimulator batch(n, B), other(n, B2);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    other.setNoiseSemantics(qsim::BatchedNoise::Physical);
    batch.runSweep(ansatz(n, std::vector<double>(P, 0.1)), angles);
    other.runSweep(ansatz(n, std::vector<double>(P, 0.1)), angles2);
    const auto psi = oracle_states(n, B, angles), phi = oracle_states(n, B2, angles2);

    const std::vector<cplx> g = batch.overlapMatrix();
    const std::vector<double> k = batch.kernelMatrix();
    ASSERT_TRUE(g.size() == (size_t)B * B && k.size() == g.size());
    double worst = 0.0, worst_k = 0.0;
    bool hermitian = true;
    for (int i = 0; i < B; ++i)
        for (int j = 0; j < B; ++j) {
            const cplx want = vdot(psi[i], psi[j]);
            worst = std::max(worst, component_error(g[(size_t)i * B + j], want));
            worst_k = std::max(worst_k, std::fabs(k[(size_t)i * B + j] - std::norm(want)));
            hermitian = hermitian && g[(size_t)j * B + i].real() == g[(size_t)i * B + j].real() &&
                        g[(size_t)j * B + i].imag() == -g[(size_t)i * B + j].imag();
        }
    EXPECT_NEAR(worst, 0.0, 1e-12);
    EXPECT_NEAR(worst_k, 0.0, 4e-12);  // |x|^2 from components within 1e-12, |x| <= 1: < 3e-12
    EXPECT_TRUE(hermitian);
    for (int i = 0; i < B; ++i) EXPECT_TRUE(g[(size_t)i * B + i].imag() == 0.0 && !std::signbit(g[(size_t)i * B + i].imag()));

    const std::vector<cplx> x = batch.overlapMatrix(other);
    const std::vector<double> kx = batch.kernelMatrix(other);
    ASSERT_TRUE(x.size() == (size_t)B * B2 && kx.size() == x.size());
    worst = worst_k = 0.0;
    for (int i = 0; i < B; ++i)
        for (int j = 0; j < B2; ++j) {
            const cplx want = vdot(psi[i], phi[j]);
            worst = std::max(worst, component_error(x[(size_t)i * B2 + j], want));
            worst_k = std::max(worst_k, std::fabs(kx[(size_t)i * B2 + j] - std::norm(want)));
        }
    EXPECT_NEAR(worst, 0.0, 1e-12);
    EXPECT_NEAR(worst_k, 0.0, 4e-12);

    // one state against every trajectory: a simulator that ran trajectory 1's circuit, and a host vector
    qsim::Simulator sim(n);
    sim.run(ansatz(n, std::vector<double>(angles.begin() + P, angles.begin() + 2 * P)));
    const std::vector<cplx> v = batch.overlapsWith(sim.state());
    ASSERT_TRUE(v.size() == (size_t)B);
    worst = 0.0;
    for (int t = 0; t < B; ++t) worst = std::max(worst, component_error(v[t], vdot(psi[t], psi[1])));
    EXPECT_NEAR(worst, 0.0, 1e-12);
    EXPECT_NEAR(component_error(v[1], cplx(1.0, 0.0)), 0.0, 1e-12);
    qsim::StateVector host(n);
    host.fromHost(phi[0]);
    const std::vector<cplx> w = batch.overlapsWith(host);
    worst = 0.0;
    for (int t = 0; t < B; ++t) worst = std::max(worst, component_error(w[t], vdot(psi[t], phi[0])));
    EXPECT_NEAR(worst, 0.0, 1e-12);
}

TEST(BatchOverlap, FiveQubitsSeventeenMembers) { check_shape(5, 17, 3); }
TEST(BatchOverlap, TenQubitsFourMembers) { check_shape(10, 4, 6); }

TEST(BatchOverlap, Exceptions) {
    qsim::BatchedSimulator a(5, 4), b(6, 3);
    qsim::StateVector s(6);
    EXPECT_THROW(a.overlapMatrix(b), std::invalid_argument);
    EXPECT_THROW(a.kernelMatrix(b), std::invalid_argument);
    EXPECT_THROW(a.overlapsWith(s), std::invalid_argument);
    // both still work: every trajectory is |0...0>
    const std::vector<cplx> g = a.overlapMatrix();
    ASSERT_TRUE(g.size() == 16u);
    for (const cplx& e : g) EXPECT_TRUE(e == cplx(1.0, 0.0));
    EXPECT_NEAR(b.kernelMatrix()[4], 1.0, 0.0);
    EXPECT_NO_THROW(a.overlapMatrix(a));
}

TH_MAIN
