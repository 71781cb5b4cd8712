// test_expectation.cpp — the Pauli-sum expectation API of the C++17 layer
// (include/qsim/Observable.hpp): known answers, a 12-qubit random sum against the parity oracle
// (oracle/cpu_simulator.hpp) with the Paulis applied on the host, and the exception types.
#include <qsim/Circuit.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

#include "cpu_simulator.hpp"
#include "harness.hpp"

using cplx = std::complex<double>;
using Factors = std::vector<std::pair<int, char>>;

static double ev(const qsim::Simulator& sim, const Factors& f) {
    qsim::PauliSum h(sim.getNumQubits());
    h.add(1.0, f);
    return sim.expectation(h);
}

// sum_t c_t Re <psi|P_t|psi>, P|i> = i^nY (-1)^popcount(i & z) |i ^ x>
static double host_expectation(const std::vector<cplx>& psi, const qsim::PauliSum& h) {
    static const cplx kPhase[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
    double e = 0.0;
    for (const qsim::PauliSum::Term& t : h.terms()) {
        const cplx phase = kPhase[__builtin_popcountll(t.x_mask & t.z_mask) & 3];
        cplx acc = 0.0;
        for (size_t i = 0; i < psi.size(); ++i) {
            const double s = __builtin_popcountll(i & t.z_mask) & 1 ? -1.0 : 1.0;
            acc += std::conj(psi[i ^ t.x_mask]) * (phase * s * psi[i]);
        }
        e += t.coeff * acc.real();
    }
    return e;
}

TEST(Expectation, KnownAnswers) {
    const double tol = 1e-12;
    {
        qsim::Simulator s(1);
        EXPECT_NEAR(ev(s, {{0, 'Z'}}), 1.0, tol);
        qsim::Circuit c(1);
        c.h(0);
        s.run(c);
        EXPECT_NEAR(ev(s, {{0, 'X'}}), 1.0, tol);
    }
    {
        qsim::Simulator s(1);
        qsim::Circuit c(1);
        c.h(0).s(0);
        s.run(c);
        EXPECT_NEAR(ev(s, {{0, 'Y'}}), 1.0, tol);
    }
    {
        qsim::Simulator s(2);
        s.run(qsim::createBellCircuit());
        EXPECT_NEAR(ev(s, {{0, 'X'}, {1, 'X'}}), 1.0, tol);
        EXPECT_NEAR(ev(s, {{0, 'Y'}, {1, 'Y'}}), -1.0, tol);
        EXPECT_NEAR(ev(s, {{0, 'Z'}, {1, 'Z'}}), 1.0, tol);
        EXPECT_NEAR(ev(s, {{0, 'X'}, {1, 'Z'}}), 0.0, tol);
        EXPECT_NEAR(ev(s, {}), 1.0, tol);
    }
    {
        qsim::Simulator s(3);
        s.run(qsim::createGHZCircuit(3));
        EXPECT_NEAR(ev(s, {{0, 'X'}, {1, 'X'}, {2, 'X'}}), 1.0, tol);
        EXPECT_NEAR(ev(s, {{0, 'X'}, {1, 'Y'}, {2, 'Y'}}), -1.0, tol);
    }
}

static qsim::PauliSum random_sum(int n, int count, unsigned seed, double* abs_sum) {
    std::mt19937 rng(seed);
    qsim::PauliSum h(n);
    *abs_sum = 0.0;
    const char letters[3] = {'X', 'Y', 'Z'};
    for (int t = 0; t < count; ++t) {
        Factors f;
        for (int q = 0; q < n; ++q)
            if (rng() % 3 == 0) f.emplace_back(q, letters[rng() % 3]);
        const double c = (double)(rng() % 2001) / 1000.0 - 1.0;
        h.add(c, f);
        *abs_sum += std::fabs(c);
    }
    return h;
}

TEST(Expectation, RandomSumMatchesOracle12) {
    const int n = 12;
    const qsim::Circuit c = qsim::createRandomCircuit(n, 120, 5);
    qsim_oracle::CPUSimulator cpu(n);
    cpu.run(c);
    double abs_sum = 0.0;
    const qsim::PauliSum h = random_sum(n, 40, 17, &abs_sum);
    EXPECT_EQ(h.size(), (size_t)40);
    const double want = host_expectation(cpu.getStateVector(), h);
    for (qsim::RunMode m : {qsim::RunMode::PerGate, qsim::RunMode::Fused}) {
        qsim::Simulator sim(n);
        sim.setRunMode(m);
        sim.run(c);
        const double got = sim.expectation(h);
        EXPECT_NEAR(got, want, 1e-12 * abs_sum);
        EXPECT_NEAR(sim.state().expectation(h), got, 0.0);  // bitwise reproducible
        EXPECT_NEAR(got, host_expectation(sim.getStateVector(), h), 1e-12 * abs_sum);
    }
    qsim::NoisySimulator noisy(n);
    noisy.run(c);
    EXPECT_NEAR(noisy.expectation(h), want, 1e-12 * abs_sum);
    qsim::BatchedSimulator batch(n, 3);
    batch.run(c);
    const std::vector<double> e = batch.getExpectations(h);
    ASSERT_TRUE(e.size() == 3);
    for (double v : e) EXPECT_NEAR(v, want, 1e-12 * abs_sum);
    EXPECT_NEAR(batch.getAverageExpectation(h), ((e[0] + e[1]) + e[2]) / 3.0, 0.0);
}

TEST(Expectation, Exceptions) {
    EXPECT_THROW(qsim::PauliSum(0), std::invalid_argument);
    qsim::PauliSum h(4);
    EXPECT_THROW(h.add(1.0, {{4, 'X'}}), std::out_of_range);
    EXPECT_THROW(h.add(1.0, {{-1, 'Z'}}), std::out_of_range);
    EXPECT_THROW(h.add(1.0, {{1, 'X'}, {1, 'Z'}}), std::invalid_argument);
    EXPECT_THROW(h.add(1.0, {{1, 'Q'}}), std::invalid_argument);
    EXPECT_EQ(h.size(), (size_t)0);
    h.add(0.5, {{0, 'X'}, {3, 'Y'}});
    EXPECT_EQ(h.size(), (size_t)1);
    EXPECT_EQ(h.terms()[0].x_mask, (uint64_t)0b1001);
    EXPECT_EQ(h.terms()[0].z_mask, (uint64_t)0b1000);
    qsim::Simulator sim(5);
    EXPECT_THROW(sim.expectation(h), std::invalid_argument);
    qsim::NoisySimulator noisy(5);
    EXPECT_THROW(noisy.expectation(h), std::invalid_argument);
    qsim::BatchedSimulator batch(5, 2);
    EXPECT_THROW(batch.getExpectations(h), std::invalid_argument);
    qsim::Simulator ok(4);
    EXPECT_NEAR(ok.expectation(qsim::PauliSum(4)), 0.0, 0.0);  // no terms: 0
}

TH_MAIN
