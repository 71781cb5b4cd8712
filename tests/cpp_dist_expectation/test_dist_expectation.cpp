// test_dist_expectation.cpp — qsim::DistributedSimulator::expectation
// (include/qsim/DistributedSimulator.hpp): 8 virtual ranks at 12 qubits after a GHZ and a random
// circuit — known answers, equality with Simulator::expectation at 1e-12 * sum |c|, the value's
// reproducibility and the exception type.
#include <qsim/Circuit.hpp>
#include <qsim/DistributedSimulator.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>

#include <cmath>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

#include "harness.hpp"

using Factors = std::vector<std::pair<int, char>>;

static double ev(const qsim::DistributedSimulator& d, const Factors& f) {
    qsim::PauliSum h(d.getNumQubits());
    h.add(1.0, f);
    return d.expectation(h);
}

TEST(DistExpectation, GhzKnownAnswers) {
    const int n = 12;
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    d.run(qsim::createGHZCircuit(n));
    const double tol = 1e-12;
    Factors all_x, xyy;
    for (int q = 0; q < n; ++q) all_x.push_back({q, 'X'});
    EXPECT_NEAR(ev(d, all_x), 1.0, tol);  // X on every qubit: local and rank positions alike
    for (int q = 0; q + 1 < n; ++q) EXPECT_NEAR(ev(d, {{q, 'Z'}, {q + 1, 'Z'}}), 1.0, tol);
    EXPECT_NEAR(ev(d, {{0, 'Z'}, {n - 1, 'Z'}}), 1.0, tol);
    for (int q = 0; q < n; ++q) {
        EXPECT_NEAR(ev(d, {{q, 'Z'}}), 0.0, tol);
        EXPECT_NEAR(ev(d, {{q, 'X'}}), 0.0, tol);
    }
    // two Y among the X: -1, wherever the Y sit
    for (int a : {0, 5, n - 2}) {
        Factors f = all_x;
        f[a].second = 'Y';
        f[n - 1].second = 'Y';
        EXPECT_NEAR(ev(d, f), -1.0, tol);
    }
    EXPECT_NEAR(ev(d, {}), 1.0, tol);  // identity: the norm
    // a second run moves the map on; the answers stay
    d.reset();
    d.run(qsim::createRandomHCCircuit(n, 100, 42));
    d.reset();
    d.run(qsim::createGHZCircuit(n));
    EXPECT_NEAR(ev(d, all_x), 1.0, tol);
}

TEST(DistExpectation, MatchesSimulator) {
    const int n = 12;
    const qsim::Circuit c = qsim::createRandomCircuit(n, 100, 5);
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::Simulator sim(n);
    for (int rep = 0; rep < 2; ++rep) {
        d.run(c);
        sim.run(c);
    }
    std::mt19937_64 rng(99);
    std::uniform_real_distribution<double> coeff(-1.0, 1.0);
    const char letters[4] = {'I', 'X', 'Y', 'Z'};
    qsim::PauliSum h(n);
    double sum_abs = 0.0;
    for (int t = 0; t < 40; ++t) {
        Factors f;
        for (int q = 0; q < n; ++q) {
            const int l = (int)(rng() & 3);
            // (half of the terms X/Y-free below qubit 6, so several share an x mask)
            if (l == 0 || (t % 2 == 0 && q < 6 && l != 3)) continue;
            f.push_back({q, letters[l]});
        }
        const double cf = coeff(rng);
        sum_abs += std::fabs(cf);
        h.add(cf, f);
    }
    const std::vector<std::complex<double>> before = d.getStateVector();
    const double a = d.expectation(h);
    EXPECT_NEAR(a, sim.expectation(h), 1e-12 * sum_abs);
    EXPECT_TRUE(d.expectation(h) == a);  // fixed-order sums: bit for bit
    EXPECT_TRUE(d.getStateVector() == before);
    // every single string too
    for (const qsim::PauliSum::Term& t : h.terms()) {
        qsim::PauliSum one(n);
        Factors f;
        for (int q = 0; q < n; ++q) {
            const bool x = t.x_mask >> q & 1, z = t.z_mask >> q & 1;
            if (x || z) f.push_back({q, x && z ? 'Y' : (x ? 'X' : 'Z')});
        }
        one.add(1.0, f);
        EXPECT_NEAR(d.expectation(one), sim.expectation(one), 1e-12);
    }
}

TEST(DistExpectation, Exceptions) {
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(12, 8);
    qsim::PauliSum wrong(11);
    wrong.add(1.0, {{0, 'X'}});
    EXPECT_THROW(d.expectation(wrong), std::invalid_argument);
    qsim::PauliSum empty(12);
    EXPECT_NEAR(d.expectation(empty), 0.0, 0.0);
    qsim::PauliSum z(12);
    z.add(2.0, {{11, 'Z'}});
    EXPECT_NEAR(d.expectation(z), 2.0, 1e-15);  // |0..0>
}

TH_MAIN
