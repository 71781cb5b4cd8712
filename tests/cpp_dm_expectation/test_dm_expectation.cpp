// test_dm_expectation.cpp — Re Tr(rho H) through the C++17 layer (include/qsim/DensityMatrix.hpp,
// include/qsim/Observable.hpp): closed-form answers with and without a depolarizing channel, the
// exception on a qubit-count mismatch, DensityMatrix against DensityMatrixSimulator.
#include <qsim/Circuit.hpp>
#include <qsim/DensityMatrix.hpp>
#include <qsim/NoiseModel.hpp>
#include <qsim/Observable.hpp>

#include <stdexcept>
#include <utility>
#include <vector>

#include "harness.hpp"

using Factors = std::vector<std::pair<int, char>>;

static qsim::PauliSum one(int n, const Factors& f, double c = 1.0) {
    qsim::PauliSum h(n);
    h.add(c, f);
    return h;
}

TEST(DmExpectation, KnownAnswers) {
    const double tol = 1e-12;
    const int n = 4;
    for (int q = 0; q < n; ++q) {
        qsim::DensityMatrixSimulator sim(n);  // |0><0|
        EXPECT_NEAR(sim.expectation(one(n, {{q, 'Z'}})), 1.0, tol);
        EXPECT_NEAR(sim.expectation(one(n, {{q, 'X'}})), 0.0, tol);
        EXPECT_NEAR(sim.expectation(one(n, {}, 0.5)), 0.5, tol);
        qsim::Circuit c(n);
        c.h(q);
        sim.run(c);
        EXPECT_NEAR(sim.expectation(one(n, {{q, 'X'}})), 1.0, tol);
        EXPECT_NEAR(sim.expectation(one(n, {{q, 'Z'}})), 0.0, tol);
        EXPECT_NEAR(sim.expectation(one(n, {{q, 'Y'}})), 0.0, tol);
    }
}

TEST(DmExpectation, DepolarizingScalesX) {
    const int n = 3;
    for (int q = 0; q < n; ++q) {
        for (double p : {0.0, 0.03, 0.3}) {
            qsim::NoiseModel noise;
            noise.addDepolarizing({q}, p);
            qsim::DensityMatrixSimulator sim(n, noise);
            qsim::Circuit c(n);
            c.h(q);
            sim.run(c);  // H, then the channel on q: the off-diagonal elements scale by 1 - 4p/3
            EXPECT_NEAR(sim.expectation(one(n, {{q, 'X'}})), 1.0 - 4.0 * p / 3.0, 1e-12);
            EXPECT_NEAR(sim.expectation(one(n, {})), 1.0, 1e-12);
        }
    }
}

TEST(DmExpectation, MatrixAndSimulatorAgree) {
    const int n = 5;
    qsim::NoiseModel noise;
    noise.addDepolarizing(0.02);
    noise.addAmplitudeDamping({1}, 0.1);
    qsim::DensityMatrixSimulator sim(n, noise);
    qsim::Circuit c(n);
    c.h(0).cnot(0, 1).ry(2, 0.4).rx(3, 1.1).cz(2, 3).s(1).h(4).cnot(4, 2);
    sim.run(c);
    qsim::PauliSum h(n);
    h.add(0.5, {{0, 'X'}, {1, 'Y'}}).add(-1.25, {{2, 'Z'}, {3, 'Z'}}).add(0.75, {{4, 'Y'}}).add(2.0, {});
    const double a = sim.expectation(h);
    EXPECT_NEAR(sim.density().expectation(h), a, 0.0);  // the same reduction: bitwise equal
    EXPECT_NEAR(sim.expectation(h), a, 0.0);
    qsim::DensityMatrix mixed(n);
    mixed.initMaximallyMixed();
    EXPECT_NEAR(mixed.expectation(h), 2.0, 1e-12);  // only the identity term survives
    EXPECT_NEAR(mixed.expectation(qsim::PauliSum(n)), 0.0, 0.0);  // no terms: 0
}

TEST(DmExpectation, Exceptions) {
    qsim::PauliSum h(4);
    h.add(1.0, {{0, 'Z'}});
    qsim::DensityMatrixSimulator sim(5);
    EXPECT_THROW(sim.expectation(h), std::invalid_argument);
    qsim::DensityMatrix rho(3);
    EXPECT_THROW(rho.expectation(h), std::invalid_argument);
}

TH_MAIN
