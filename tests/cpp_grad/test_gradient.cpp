// test_gradient.cpp — the adjoint-gradient API of the C++17 layer: Simulator::gradient against closed
// forms and against the exact +-pi/2 parameter shift through run() + expectation(),
// StateVector::applyPauliSum / innerProduct against the host, and the exception types.
#include <qsim/Circuit.hpp>
#include <qsim/Observable.hpp>
#include <qsim/Simulator.hpp>
#include <qsim/StateVector.hpp>

#include <cmath>
#include <complex>
#include <stdexcept>
#include <utility>
#include <vector>

#include "harness.hpp"

using cplx = std::complex<double>;

TEST(Gradient, ClosedForms) {
    const double th = 0.73, tol = 1e-12;
    qsim::PauliSum z(1);
    z.add(1.0, {{0, 'Z'}});
    {
        qsim::Simulator s(1);
        qsim::Circuit c(1);
        c.ry(0, th);
        const qsim::Gradient g = s.gradient(c, z);
        EXPECT_NEAR(g.value, std::cos(th), tol);
        ASSERT_TRUE(g.gradient.size() == 1);
        EXPECT_NEAR(g.gradient[0], -std::sin(th), tol);
        EXPECT_NEAR(s.expectation(z), g.value, 0.0);  // the state holds U|psi0>
    }
    {
        qsim::Simulator s(1);
        qsim::Circuit c(1);
        c.rz(0, th);
        const qsim::Gradient g = s.gradient(c, z, qsim::RunMode::PerGate);
        EXPECT_NEAR(g.value, 1.0, tol);
        EXPECT_NEAR(g.gradient[0], 0.0, tol);
    }
    {
        qsim::Simulator s(2);
        qsim::PauliSum z1(2);
        z1.add(1.0, {{1, 'Z'}});
        qsim::Circuit c(2);
        c.x(0).cry(0, 1, th);
        const qsim::Gradient g = s.gradient(c, z1);
        ASSERT_TRUE(g.gradient.size() == 2);
        EXPECT_NEAR(g.value, std::cos(th), tol);
        EXPECT_NEAR(g.gradient[0], 0.0, 0.0);  // X has no parameter
        EXPECT_NEAR(g.gradient[1], -std::sin(th), tol);
    }
}

static qsim::Circuit ansatz(int n, const std::vector<double>& angles) {
    qsim::Circuit c(n);
    size_t a = 0;
    for (int layer = 0; layer < 2; ++layer) {
        for (int q = 0; q < n; ++q) c.ry(q, angles[a++]);
        for (int q = 0; q < n; ++q) c.rz(q, angles[a++]);
        for (int q = 0; q + 1 < n; ++q) c.cnot(q, q + 1);
    }
    for (int q = 0; q < n; ++q) c.rx(q, angles[a++]);
    return c;
}

TEST(Gradient, MatchesParameterShift8) {
    const int n = 8;
    std::vector<double> angles(5 * n);
    for (size_t i = 0; i < angles.size(); ++i) angles[i] = 0.1 + 0.37 * (double)i;
    qsim::PauliSum h(n);
    double abs_sum = 0.0;
    for (int q = 0; q + 1 < n; ++q) {
        h.add(-1.0, {{q, 'Z'}, {q + 1, 'Z'}});
        abs_sum += 1.0;
    }
    for (int q = 0; q < n; ++q) {
        h.add(-0.5, {{q, 'X'}});
        abs_sum += 0.5;
    }
    h.add(0.25, {{0, 'Y'}, {3, 'X'}, {5, 'Y'}});
    abs_sum += 0.25;
    const qsim::Circuit c = ansatz(n, angles);
    for (qsim::RunMode m : {qsim::RunMode::Fused, qsim::RunMode::PerGate}) {
        qsim::Simulator sim(n);
        const qsim::Gradient g = sim.gradient(c, h, m);
        ASSERT_TRUE(g.gradient.size() == c.getGates().size());
        qsim::Simulator plain(n);
        plain.setRunMode(m);
        plain.run(c);
        EXPECT_NEAR(g.value, plain.expectation(h), 1e-12 * abs_sum);
        EXPECT_NEAR(sim.state().maxAbsDiff(plain.state()), 0.0, 0.0);
        size_t a = 0;
        for (size_t k = 0; k < c.getGates().size(); ++k) {
            const qsim::GateOp& gate = c.getGates()[k];
            if (gate.type == qsim::GateType::CNOT) {
                EXPECT_NEAR(g.gradient[k], 0.0, 0.0);
                continue;
            }
            double e[2];
            for (int side = 0; side < 2; ++side) {
                std::vector<double> shifted = angles;
                shifted[a] += side == 0 ? M_PI / 2 : -M_PI / 2;
                qsim::Simulator s(n);
                s.setRunMode(m);
                s.run(ansatz(n, shifted));
                e[side] = s.expectation(h);
            }
            EXPECT_NEAR(g.gradient[k], (e[0] - e[1]) / 2, 1e-12 * abs_sum);
            ++a;
        }
        EXPECT_EQ(a, angles.size());
        const qsim::Gradient again = qsim::Simulator(n).gradient(c, h, m);
        for (size_t k = 0; k < g.gradient.size(); ++k) EXPECT_NEAR(again.gradient[k], g.gradient[k], 0.0);
        sim.releaseGradientBuffers();
    }
}

TEST(Gradient, ApplyPauliSumAndInnerProduct) {
    const int n = 10;
    qsim::Simulator sim(n);
    sim.run(qsim::createRandomCircuit(n, 100, 9));
    qsim::PauliSum h(n);
    h.add(0.7, {{0, 'X'}, {9, 'Y'}}).add(-0.4, {{3, 'Z'}}).add(0.2, {{0, 'X'}, {4, 'Z'}}).add(1.5, {});
    const double abs_sum = 0.7 + 0.4 + 0.2 + 1.5;
    qsim::StateVector dst(n);
    sim.state().applyPauliSum(h, dst);
    const std::vector<cplx> psi = sim.getStateVector(), got = dst.toHost();
    static const cplx kPhase[4] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};
    std::vector<cplx> want(psi.size(), cplx(0, 0));
    for (const qsim::PauliSum::Term& t : h.terms())
        for (size_t i = 0; i < psi.size(); ++i) {
            const size_t j = i ^ t.x_mask;
            const double s = __builtin_popcountll(j & t.z_mask) & 1 ? -1.0 : 1.0;
            want[i] += t.coeff * kPhase[__builtin_popcountll(t.x_mask & t.z_mask) & 3] * s * psi[j];
        }
    double worst = 0.0;
    cplx dot = 0.0;
    for (size_t i = 0; i < psi.size(); ++i) {
        worst = std::fmax(worst, std::fmax(std::fabs(got[i].real() - want[i].real()),
                                           std::fabs(got[i].imag() - want[i].imag())));
        dot += std::conj(psi[i]) * want[i];
    }
    EXPECT_NEAR(worst, 0.0, 1e-12 * abs_sum);
    const cplx ip = sim.state().innerProduct(dst);
    EXPECT_NEAR(ip.real(), dot.real(), 1e-12 * abs_sum);
    EXPECT_NEAR(ip.imag(), dot.imag(), 1e-12 * abs_sum);
    EXPECT_NEAR(ip.real(), sim.expectation(h), 1e-12 * abs_sum);
    const cplx norm = sim.state().innerProduct(sim.state());
    EXPECT_NEAR(norm.real(), sim.state().getTotalProbability(), 1e-12);
    EXPECT_NEAR(norm.imag(), 0.0, 1e-12);
    const cplx twice = sim.state().innerProduct(dst);
    EXPECT_NEAR(twice.real(), ip.real(), 0.0);  // bitwise reproducible
    EXPECT_NEAR(twice.imag(), ip.imag(), 0.0);
}

TEST(Gradient, Exceptions) {
    qsim::Simulator sim(4);
    qsim::PauliSum h4(4), h5(5);
    h4.add(1.0, {{0, 'Z'}});
    qsim::Circuit c4(4), c5(5);
    c4.rx(0, 0.3);
    EXPECT_THROW(sim.gradient(c5, h4), std::invalid_argument);
    EXPECT_THROW(sim.gradient(c4, h5), std::invalid_argument);
    qsim::StateVector other(5), same(4);
    EXPECT_THROW(sim.state().applyPauliSum(h4, other), std::invalid_argument);
    EXPECT_THROW(sim.state().applyPauliSum(h4, sim.state()), std::invalid_argument);
    EXPECT_THROW(sim.state().applyPauliSum(h5, same), std::invalid_argument);
    EXPECT_THROW(sim.state().innerProduct(other), std::invalid_argument);
    const qsim::Gradient none = sim.gradient(c4, qsim::PauliSum(4));  // no terms: zeros
    EXPECT_NEAR(none.value, 0.0, 0.0);
    ASSERT_TRUE(none.gradient.size() == 1);
    EXPECT_NEAR(none.gradient[0], 0.0, 0.0);
    const qsim::Gradient empty = sim.gradient(qsim::Circuit(4), h4);  // no gates: <H> as it is
    EXPECT_EQ(empty.gradient.size(), (size_t)0);
    EXPECT_NEAR(empty.value, sim.expectation(h4), 0.0);
}

TH_MAIN
