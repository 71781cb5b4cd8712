// test_batch_sweep.cpp — BatchedSimulator::runSweep of the C++17 layer: one circuit, one angle set
// per trajectory, against the header-only CPU oracle (oracle/cpu_simulator.hpp) run once per
// trajectory with that trajectory's angles written into the circuit, and the exception types.
#include <qsim/Circuit.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Observable.hpp>

#include <cmath>
#include <complex>
#include <random>
#include <stdexcept>
#include <vector>

#include "cpu_simulator.hpp"
#include "harness.hpp"

using cplx = std::complex<double>;

// The test circuit with the angle set `a` (7 parameterised gates; both control orders).
static qsim::Circuit ansatz(int n, const std::vector<double>& a) {
    qsim::Circuit c(n);
    for (int q = 0; q < n; ++q) c.h(q);
    c.rx(0, a[0]).ry(n - 1, a[1]).rz(4, a[2]);
    for (int q = 0; q + 1 < n; ++q) c.cnot(q, q + 1);
    c.cry(1, n - 2, a[3]).crz(n - 1, 2, a[4]).t(3).toffoli(0, 5, 7);
    c.ry(6, a[5]).rz(0, a[6]).swap(2, n - 1);
    return c;
}

// <psi| sum_t c_t P_t |psi> on the host; P = i^(#Y) X^x Z^z.
static double host_expectation(const std::vector<cplx>& psi, const qsim::PauliSum& h) {
    double total = 0.0;
    for (const qsim::PauliSum::Term& t : h.terms()) {
        static const cplx ipow[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
        const cplx ph = ipow[__builtin_popcountll(t.x_mask & t.z_mask) & 3];
        cplx acc = 0.0;
        for (uint64_t j = 0; j < psi.size(); ++j) {
            const double sign = (__builtin_popcountll(t.z_mask & j) & 1) ? -1.0 : 1.0;
            acc += std::conj(psi[j ^ t.x_mask]) * ph * sign * psi[j];
        }
        total += t.coeff * acc.real();
    }
    return total;
}

TEST(BatchSweep, MatchesOraclePerTrajectory) {
    const int n = 10, B = 3, P = 7;
    std::mt19937 rng(11);
    std::uniform_real_distribution<double> dist(-3.0, 3.0);
    std::vector<double> angles((size_t)B * P);
    for (double& v : angles) v = dist(rng);
    qsim::PauliSum h(n);
    h.add(0.7, {{0, 'Z'}, {9, 'Z'}}).add(-0.4, {{1, 'X'}, {5, 'Y'}}).add(0.3, {{8, 'Y'}}).add(0.2, {{2, 'X'}, {3, 'Z'}});
    qsim::BatchedSimulator batch(n, B);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    // the angles stored in the circuit are ignored
    batch.runSweep(ansatz(n, std::vector<double>(P, 0.123)), angles);
    const std::vector<double> e = batch.getExpectations(h);
    ASSERT_TRUE(e.size() == (size_t)B);
    for (int t = 0; t < B; ++t) {
        qsim_oracle::CPUSimulator cpu(n);
        cpu.run(ansatz(n, std::vector<double>(angles.begin() + t * P, angles.begin() + (t + 1) * P)));
        const std::vector<cplx>& psi = cpu.getStateVector();
        const std::vector<double> p = batch.getProbabilities(t);
        ASSERT_TRUE(p.size() == psi.size());
        double worst = 0.0;
        for (size_t i = 0; i < p.size(); ++i) worst = std::max(worst, std::fabs(p[i] - std::norm(psi[i])));
        EXPECT_NEAR(worst, 0.0, 1e-12);
        EXPECT_NEAR(e[t], host_expectation(psi, h), 1e-12 * 1.6);
    }
}

TEST(BatchSweep, Exceptions) {
    const int n = 10, B = 3, P = 7;
    const qsim::Circuit c = ansatz(n, std::vector<double>(P, 0.5));
    qsim::BatchedSimulator batch(n, B);
    // the default noise semantics is the reference's
    EXPECT_THROW(batch.runSweep(c, std::vector<double>((size_t)B * P, 0.1)), std::invalid_argument);
    batch.setNoiseSemantics(qsim::BatchedNoise::Physical);
    EXPECT_THROW(batch.runSweep(c, std::vector<double>((size_t)B * P - 1, 0.1)), std::invalid_argument);
    EXPECT_THROW(batch.runSweep(c, std::vector<double>((size_t)P, 0.1)), std::invalid_argument);
    EXPECT_THROW(batch.runSweep(qsim::Circuit(n + 1), {}), std::invalid_argument);
    qsim::NoiseModel nm;
    nm.addDepolarizing({0}, 0.1);
    batch.setNoiseModel(nm);
    EXPECT_THROW(batch.runSweep(c, std::vector<double>((size_t)B * P, 0.1)), std::invalid_argument);
    batch.setNoiseModel(qsim::NoiseModel());
    batch.setGateSet(qsim::BatchedGateSet::Reference);
    EXPECT_THROW(batch.runSweep(c, std::vector<double>((size_t)B * P, 0.1)), std::invalid_argument);
    batch.setGateSet(qsim::BatchedGateSet::Full);
    // nothing ran: every trajectory is still |0...0>
    const std::vector<double> p = batch.getProbabilities(1);
    EXPECT_NEAR(p[0], 1.0, 0.0);
    batch.runSweep(c, std::vector<double>((size_t)B * P, 0.1));  // and the object still works
    EXPECT_NEAR(batch.getAverageProbabilities().size(), (double)(1u << n), 0.0);
}

TH_MAIN
