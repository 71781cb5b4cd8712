// test_dist_gradient.cpp — qsim::DistributedSimulator::gradient
// (include/qsim/DistributedSimulator.hpp) on 8 virtual ranks at 12 qubits: closed forms with the
// rotations on local and on rank positions, equality with Simulator::gradient at 1e-12 * sum |c|,
// the result's reproducibility, the state after the call and the exception type.
#include <qsim/Circuit.hpp>
#include <qsim/DistributedSimulator.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>

#include <cmath>
#include <stdexcept>
#include <vector>

#include "harness.hpp"

// Ry(t_q) on every qubit of |0..0>, H = sum_q Z_q: E = sum cos t_q, dE/dt_q = -sin t_q.  The
// forward run brings each Ry's target to a local position, so under the map it ends with other
// rotations sit on rank positions: the sweep pairs ranks for those.
TEST(DistGradient, RyZClosedForm) {
    const int n = 12;
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::Circuit c(n);
    qsim::PauliSum h(n);
    double want = 0.0;
    for (int q = 0; q < n; ++q) {
        c.ry(q, 0.2 + 0.25 * q);
        h.add(1.0, {{q, 'Z'}});
        want += std::cos(0.2 + 0.25 * q);
    }
    for (int q = 0; q + 1 < n; ++q) c.cz(q, q + 1);  // diagonal: commutes with every Z
    const qsim::Gradient g = d.gradient(c, h);
    EXPECT_NEAR(g.value, want, 1e-12 * n);
    EXPECT_TRUE((int)g.gradient.size() == 2 * n - 1);
    for (int q = 0; q < n; ++q) EXPECT_NEAR(g.gradient[q], -std::sin(0.2 + 0.25 * q), 1e-12 * n);
    for (int q = n; q < 2 * n - 1; ++q) EXPECT_TRUE(g.gradient[q] == 0.0);
}

// Rx(t)|0> has <Y> = -sin t; X on the control, then CRY(t) of |0> has <Z> = cos t; Rz(a) after an
// H has <X> = cos a.  Targets 9 .. 11 start on rank positions.
TEST(DistGradient, RxCryRzClosedForms) {
    const int n = 12;
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::Circuit c(n);
    qsim::PauliSum h(n);
    c.x(0).h(5).h(10);
    c.rx(11, 0.7).rx(2, -0.4).cry(0, 9, 1.1).cry(0, 3, 0.3).rz(5, 0.9).rz(10, -0.6);
    h.add(1.0, {{11, 'Y'}}).add(1.0, {{2, 'Y'}}).add(1.0, {{9, 'Z'}}).add(1.0, {{3, 'Z'}});
    h.add(1.0, {{5, 'X'}}).add(1.0, {{10, 'X'}});
    const qsim::Gradient g = d.gradient(c, h);
    const double tol = 6e-12;
    EXPECT_NEAR(g.value, -std::sin(0.7) - std::sin(-0.4) + std::cos(1.1) + std::cos(0.3) + std::cos(0.9) + std::cos(-0.6), tol);
    EXPECT_NEAR(g.gradient[3], -std::cos(0.7), tol);
    EXPECT_NEAR(g.gradient[4], -std::cos(-0.4), tol);
    EXPECT_NEAR(g.gradient[5], -std::sin(1.1), tol);
    EXPECT_NEAR(g.gradient[6], -std::sin(0.3), tol);
    EXPECT_NEAR(g.gradient[7], -std::sin(0.9), tol);
    EXPECT_NEAR(g.gradient[8], -std::sin(-0.6), tol);
}

TEST(DistGradient, MatchesSimulator) {
    const int n = 12;
    const qsim::Circuit pre = qsim::createRandomHCCircuit(n, 100, 42);
    qsim::Circuit c(n);
    for (int q = 0; q < n; ++q) c.ry(q, 0.1 * (q + 1)).rz(q, -0.07 * (q + 2));
    for (int q = 0; q + 1 < n; ++q) c.cnot(q, q + 1);
    for (int q = 0; q < n; ++q) c.rx(q, 0.05 * (q + 3));
    c.cry(11, 0, 0.4).crz(1, 10, -0.8).toffoli(0, 1, 2).swap(3, 11).ry(3, 0.6);
    qsim::PauliSum h(n);
    double sum_abs = 0.0;
    for (int q = 0; q < n; ++q) {
        h.add(0.3 + 0.05 * q, {{q, 'Z'}, {(q + 1) % n, 'Z'}});
        h.add(-0.2 - 0.01 * q, {{q, 'X'}});
        h.add(0.15, {{q, 'Y'}, {(q + 5) % n, 'X'}});
        sum_abs += 0.3 + 0.05 * q + 0.2 + 0.01 * q + 0.15;
    }
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::DistributedSimulator twin = qsim::DistributedSimulator::makeVirtual(n, 8);
    qsim::Simulator sim(n);
    for (int rep = 0; rep < 2; ++rep) {
        d.run(pre);
        twin.run(pre);
        sim.run(pre);
    }
    const qsim::Gradient a = d.gradient(c, h);
    const qsim::Gradient want = sim.gradient(c, h);
    EXPECT_NEAR(a.value, want.value, 1e-12 * sum_abs);
    EXPECT_TRUE(a.gradient.size() == want.gradient.size());
    for (size_t k = 0; k < a.gradient.size(); ++k) EXPECT_NEAR(a.gradient[k], want.gradient[k], 1e-12 * sum_abs);
    twin.run(c);
    EXPECT_TRUE(d.getStateVector() == twin.getStateVector());  // the state: what run() alone leaves
    // per-gate mode and a second call after a release: the same values within the bar
    d.releaseGradientBuffers();
    qsim::DistributedSimulator e = qsim::DistributedSimulator::makeVirtual(n, 8);
    for (int rep = 0; rep < 2; ++rep) e.run(pre);
    const qsim::Gradient b = e.gradient(c, h, qsim::RunMode::PerGate);
    for (size_t k = 0; k < a.gradient.size(); ++k) EXPECT_NEAR(b.gradient[k], want.gradient[k], 1e-12 * sum_abs);
}

TEST(DistGradient, Exceptions) {
    qsim::DistributedSimulator d = qsim::DistributedSimulator::makeVirtual(12, 8);
    qsim::PauliSum h(12), wrong(11);
    h.add(1.0, {{0, 'Z'}});
    wrong.add(1.0, {{0, 'X'}});
    EXPECT_THROW(d.gradient(qsim::Circuit(11), h), std::invalid_argument);
    EXPECT_THROW(d.gradient(qsim::Circuit(12), wrong), std::invalid_argument);
    const qsim::Gradient g = d.gradient(qsim::Circuit(12), h);  // no gate: the value of |0..0>
    EXPECT_NEAR(g.value, 1.0, 1e-15);
    EXPECT_TRUE(g.gradient.empty());
    d.releaseGradientBuffers();  // nothing was allocated: fine
}

TH_MAIN
